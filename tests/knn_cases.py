"""The clouds of the k-NN tests (tests/test_knn_ref.py, tests/test_gpu_knn.py): each returns float32
arrays; a case with its own queries returns them after the surface."""
import numpy as np

from pcl_feature_extraction_amd.synth import synth_room

f32 = np.float32
ROOM_N = 8192
ROOM_KS = (1, 2, 3, 10, 32)          # and KNN_MAX_K
LATTICE_KS = (7, 8, 27, 30)


def room(n=ROOM_N):
    x, y, z, _ = synth_room(n, 1)
    return x, y, z


def room_queries(nq=512, seed=5):
    """Separate query points around the room: about a quarter of them outside its bounding box, a few
    of those many extents away."""
    x, y, z = room()
    rng = np.random.default_rng(seed)
    lo = np.array([x.min(), y.min(), z.min()], np.float64)
    hi = np.array([x.max(), y.max(), z.max()], np.float64)
    q = rng.uniform(lo - 0.15 * (hi - lo), hi + 0.15 * (hi - lo), (nq, 3))
    q[:8] = hi + (hi - lo) * rng.uniform(5.0, 50.0, (8, 3))
    q[8:16] = lo - (hi - lo) * rng.uniform(5.0, 50.0, (8, 3))
    q = q.astype(f32)
    outside = ((q < lo) | (q > hi)).any(axis=1)
    assert 64 < outside.sum() < nq - 64
    return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()


def lattice(m=16):
    """m^3 integer coordinates: every d2 is a small integer, so rows are full of exact ties."""
    g = np.arange(m, dtype=f32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return x.ravel().copy(), y.ravel().copy(), z.ravel().copy()


def duplicates(seed=7):
    """64 copies of one point scattered (by index) among 1,000 others."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (1064, 3)).astype(f32)
    at = np.sort(rng.choice(1064, 64, replace=False))
    p[at] = p[at[0]]
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), at


def two_densities(dense=4096, sparse=64, seed=9):
    """`dense` points in a 1 cm cube plus `sparse` spread over 10 m."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 0.01, (dense, 3)) + 5.0
    b = rng.uniform(0.0, 10.0, (sparse, 3))
    p = np.concatenate([a, b]).astype(f32)
    p = p[rng.permutation(len(p))]
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def far_origin():
    x, y, z = room()
    return x + f32(1000.0), y + f32(1000.0), z + f32(1000.0)


def identical(n=100):
    return np.full(n, 0.25, f32), np.full(n, -1.5, f32), np.full(n, 3.0, f32)


def collinear(n=1000, seed=11):
    t = np.random.default_rng(seed).uniform(0.0, 2.0, n).astype(f32)
    return t.copy(), np.full(n, 0.5, f32), np.full(n, -0.5, f32)


def coplanar(n=4096, seed=13):
    p = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 2)).astype(f32)
    return p[:, 0].copy(), p[:, 1].copy(), np.full(n, 2.0, f32)


def single():
    return np.array([1.0], f32), np.array([2.0], f32), np.array([3.0], f32)


def short(seed=15):
    p = np.random.default_rng(seed).uniform(0.0, 1.0, (5, 3)).astype(f32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def with_nonfinite(x, y, z, seed=17):
    """A tenth of the rows given a NaN, +inf or -inf in one coordinate; returns the arrays and the rows."""
    x, y, z = x.copy(), y.copy(), z.copy()
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(len(x), len(x) // 10, replace=False))
    bad = np.array([np.nan, np.inf, -np.inf], f32)
    for j, i in enumerate(rows):
        (x, y, z)[j % 3][i] = bad[(j // 3) % 3]
    return x, y, z, rows


def plane_grid(m=15):
    """m x m points of the plane z = 1 on a jittered grid (jitter keeps the covariance well away from
    a repeated eigenvalue in the plane only by chance; the smallest one is 0 either way)."""
    rng = np.random.default_rng(19)
    g = np.arange(m, dtype=np.float64) * 0.125
    x, y = np.meshgrid(g, g, indexing="ij")
    x = (x + rng.uniform(-0.03, 0.03, x.shape)).astype(f32).ravel()
    y = (y + rng.uniform(-0.03, 0.03, y.shape)).astype(f32).ravel()
    return x.copy(), y.copy(), np.full(m * m, 1.0, f32)


def contract_rows(x, y, z, qx, qy, qz, k):
    """The contract in numpy: float32 d2 = ((0 + dx^2) + dy^2) + dz^2 with dx = q - p, a lexsort by
    (d2, index) over the finite points, the first k; -1 / NaN padding; non-finite queries empty."""
    x, y, z, qx, qy, qz = (np.asarray(v, f32) for v in (x, y, z, qx, qy, qz))
    fin = np.flatnonzero(np.isfinite(x) & np.isfinite(y) & np.isfinite(z)).astype(np.int32)
    nq = len(qx)
    counts = np.zeros(nq, np.int64)
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.nan, f32)
    for q in range(nq):
        if not (np.isfinite(qx[q]) and np.isfinite(qy[q]) and np.isfinite(qz[q])):
            continue
        with np.errstate(over="ignore"):
            dx, dy, dz = qx[q] - x[fin], qy[q] - y[fin], qz[q] - z[fin]
            d = ((f32(0) + dx * dx) + dy * dy) + dz * dz
        order = np.lexsort((fin, d))[:k]
        c = len(order)
        counts[q], idx[q, :c], d2[q, :c] = c, fin[order], d[order]
    return counts, idx, d2
