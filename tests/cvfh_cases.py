"""The clouds shared by the CVFH tests (tests/test_cvfh_ref.py, test_abi_cvfh.py, test_gpu_cvfh.py,
test_cvfh_facade.py): small scenes whose clusters follow from the geometry."""
import numpy as np

F = np.float32
TOL = F(0.005) * F(3)   # PCL's default cluster tolerance and normal radius (leaf_size_ * 3)


def f32(*a):
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in a)


OFFSET = (0.3, 0.2, 1.0)   # no face's plane holds the origin, the viewpoint the normals turn to


def _finish(p, jitter, seed, shuffle):
    rng = np.random.default_rng(seed)
    p = np.asarray(p, dtype=np.float64) + OFFSET
    if jitter:
        p = p + rng.uniform(-jitter, jitter, p.shape)
    if shuffle:
        p = p[rng.permutation(len(p))]
    return f32(p[:, 0], p[:, 1], p[:, 2])


def roof(m=40, spacing=0.005, jitter=0.0005, seed=7, shuffle=True):
    """Two m x m patches at 90 degrees that meet in a crease along y (one level, one rising from its
    edge), jittered and shuffled: 2 m m points.  The crease's points have a
    high curvature; each face is one smooth cluster."""
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    i, j = i.ravel(), j.ravel()
    a = np.stack([i * spacing, j * spacing, np.zeros(i.shape)], 1)
    b = np.stack([np.zeros(i.shape), j * spacing, (i + 1) * spacing], 1)
    return _finish(np.concatenate([a, b]), jitter, seed, shuffle)


def corner(m=24, spacing=0.005, jitter=0.0005, seed=11):
    """Three m x m faces of a cube's corner, jittered and shuffled: three smooth clusters."""
    i, j = np.meshgrid(np.arange(1, m + 1), np.arange(1, m + 1), indexing="ij")
    i, j = i.ravel() * spacing, j.ravel() * spacing
    o = np.zeros(i.shape)
    p = np.concatenate([np.stack([i, j, o], 1), np.stack([o, i, j], 1), np.stack([i, o, j], 1)])
    return _finish(p, jitter, seed, True)


def strip(n=1500, rows=3, spacing=0.004, order="index", seed=3):
    """rows x n level lattice, row after row: at the default tolerance a point reaches
    three steps along the strip, so a label needs some n / 3 hops from one end to the other.  order:
    "index", "reverse" or "shuffled"."""
    j, i = np.meshgrid(np.arange(rows), np.arange(n), indexing="ij")
    p = np.stack([i.ravel() * spacing, j.ravel() * spacing, np.zeros(i.size)], 1)
    if order == "reverse":
        p = p[::-1]
    return _finish(p, 0.0, seed, order == "shuffled")


def islands(sizes=(49, 50, 51), spacing=0.004, gap=1.0):
    """Flat islands of the given sizes (8-wide lattices, filled row by row), `gap` apart along x, in
    one level plane; returns xyz and the island of every point."""
    pts, which = [], []
    for k, size in enumerate(sizes):
        e = np.arange(size)
        pts.append(np.stack([k * gap + (e % 8) * spacing, (e // 8) * spacing, np.zeros(size)], 1))
        which.append(np.full(size, k))
    x, y, z = _finish(np.concatenate(pts), 0.0, 0, False)
    return (x, y, z), np.concatenate(which)


def flat_normals(n, sign=-1.0):
    """n normals (0, 0, sign) and zero curvatures."""
    return f32(np.zeros(n), np.zeros(n), np.full(n, sign)) + f32(np.zeros(n))


def union_find_labels(x, y, z, nx, ny, nz, tolerance, eps_angle, min_points):
    """An independent numpy statement of the smooth clusters: brute-force float32 distances and dots,
    union-find, clusters numbered by their lowest index."""
    x, y, z, nx, ny, nz = f32(x, y, z, nx, ny, nz)
    n = len(x)
    tt = F(float(F(tolerance)) * float(F(tolerance)))
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in range(n):
        dx, dy, dz = x[i] - x, y[i] - y, z[i] - z
        d2 = ((F(0) + dx * dx) + dy * dy) + dz * dz
        dot = (nx[i] * nx + ny[i] * ny) + nz[i] * nz
        with np.errstate(invalid="ignore"):
            ok = (d2 < tt) & (np.abs(np.arccos(dot.astype(np.float64))) < eps_angle)
        ok[i] = False
        for j in np.nonzero(ok)[0]:
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(n)])
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    labels = np.full(n, -1, np.int32)
    row = 0
    for r in np.unique(roots):
        members = (roots == r) & finite
        if members.sum() >= min_points:
            labels[members] = row
            row += 1
    return labels


def next_f32(v, up=True):
    return np.nextafter(F(v), F(np.inf) if up else F(-np.inf))
