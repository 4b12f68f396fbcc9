"""Synthetic clouds that put a neighbour list exactly at, one below and one above a capacity of the
list build (pfx_nblist.hip) or of a consumer -- plain numpy, no GPU.

Every cloud starts with one anchor point at the origin and keeps every other coordinate positive, so
the grid origin (the cloud's minimum) is (0, 0, 0) and the cell of a point is known:
floor(p / CELL) with CELL = R * (1 + 1e-6), as pfx_grid.hip and these builders compute it in
float64.  Blobs are centred on cell centres and are smaller than half a cell, so a blob lies in one
cell; blobs of one cloud are 20 cells (1 m) apart and never see each other.  Every builder draws
from a seeded default_rng.
"""
import numpy as np

R = 0.05
CELL = R * (1.0 + 1e-6)
STEP = 20  # cells between blobs: 1 m


def cells(p, cell=CELL):
    """Integer cell coordinates (n, 3) of points (n, 3), origin at 0 (the anchor)."""
    return np.floor(np.asarray(p, np.float64) / cell).astype(np.int64)


def cell_centre(ix, iy=10, iz=10, cell=CELL):
    return (np.array([ix, iy, iz], np.float64) + 0.5) * cell


def cube(rng, k, centre, side):
    return np.asarray(centre) + rng.uniform(-0.5 * side, 0.5 * side, (k, 3))


def assemble(parts):
    """Anchor + parts -> ((x, y, z) float32, [(first row, end row) of every part])."""
    rows, at = [], 1
    for p in parts:
        rows.append((at, at + len(p)))
        at += len(p)
    pts = np.concatenate([np.zeros((1, 3))] + [np.asarray(p, np.float64) for p in parts]).astype(np.float32)
    assert (pts[1:] > 0).all()
    return (pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()), rows


def three_rows(lo, hi):
    """First, middle and last row of [lo, hi)."""
    return [lo, (lo + hi) // 2, hi - 1]


def exact_k_blob(rng, k, slot):
    """K points in a cube of side 0.025 (diagonal 0.043 < R: every point neighbours every other) on
    the centre of cell (STEP * (slot + 1), 10, 10)."""
    return cube(rng, k, cell_centre(STEP * (slot + 1)), 0.025)


def exact_k_blobs(caps, deltas=(-1, 0, 1), seed=101):
    """One blob of K = cap + delta points per (cap, delta): each of its points has exactly K
    neighbours and a 3x3x3 block of exactly K candidates.
    Returns (x, y, z), [(K, first row, end row)]."""
    rng = np.random.default_rng(seed)
    ks = [cap + d for cap in caps for d in deltas]
    xyz, rows = assemble([exact_k_blob(rng, k, s) for s, k in enumerate(ks)])
    return xyz, [(k, lo, hi) for k, (lo, hi) in zip(ks, rows)]


def two_blob_pair(rng, k_a, k_b, slot, axes=(0, 1), side=0.004):
    """Blob A (k_a points) on the centre of cell (STEP * (slot + 1), 20, 20) and blob B (k_b) 0.8
    cells further along both `axes`: diagonally adjacent cells, cubes of side 0.004 whose gap is
    sqrt(2) * (0.8 * CELL - 0.004) = 0.0509 > R.  A tile of either blob sees k_a + k_b candidates
    while its lists hold k_a or k_b entries."""
    ca = cell_centre(STEP * (slot + 1), 20, 20)
    cb = ca.copy()
    for a in axes:
        cb[a] += 0.8 * CELL
    return cube(rng, k_a, ca, side), cube(rng, k_b, cb, side)


def two_blob_blocks(pairs, seed=102):
    """For every (K_a, T): blob A of K_a and blob B of T - K_a points in diagonally adjacent cells
    (x and y), more than R apart.  Returns (x, y, z), [(K_a, T, (A rows), (B rows))]."""
    rng = np.random.default_rng(seed)
    parts = []
    for s, (k_a, t) in enumerate(pairs):
        parts.extend(two_blob_pair(rng, k_a, t - k_a, s))
    xyz, rows = assemble(parts)
    return xyz, [(k_a, t, rows[2 * s], rows[2 * s + 1]) for s, (k_a, t) in enumerate(pairs)]


def tied_shell(rng, k, centre, radius=0.02):
    """One centre point (row 0) plus k - 1 points on a sphere of `radius` around it: the centre's
    list has k entries with a few hundred distinct d2 values (float32 rounding of the shell), so
    almost all of it lands in one or two sort buckets, ordered by the caller-index tie-break."""
    v = rng.normal(size=(k - 1, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([np.asarray(centre)[None], np.asarray(centre) + radius * v])


def identical_points(k, centre):
    """k copies of one point: every d2 is 0, every list is the identity order."""
    return np.repeat(np.asarray(centre, np.float64)[None], k, axis=0)


def ties_cloud(shell_ks, identical_ks, seed=103):
    """Tied shells then identical clusters, 1 m apart.
    Returns (x, y, z), [(K, first row, end row)] in that order (a shell's first row is its centre)."""
    rng = np.random.default_rng(seed)
    parts = [tied_shell(rng, k, cell_centre(STEP * (s + 1))) for s, k in enumerate(shell_ks)]
    parts += [identical_points(k, cell_centre(STEP * (len(shell_ks) + s + 1))) for s, k in enumerate(identical_ks)]
    xyz, rows = assemble(parts)
    return xyz, [(k, lo, hi) for k, (lo, hi) in zip(list(shell_ks) + list(identical_ks), rows)]


LATTICE_R = 0.0625
LATTICE_N = 13
LATTICE_INTERIOR_COUNT = 251  # integer vectors with |v|^2 < 16 (the 6 at exactly 4 steps = r excluded)


def binary_lattice():
    """A 13^3 lattice of spacing 1/64 offset by (3.0, 1.5, 0.25), for r = 1/16: every coordinate and
    every d2 is exact in float32, so an interior point (>= 4 steps from every face) has exactly
    the neighbours v with |v|^2 < 16 -- 251 of them, whatever the oracle says.
    Returns (x, y, z), rows of the interior points."""
    i = np.arange(LATTICE_N)
    g = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    xyz, rows = assemble([g / 64.0 + np.array([3.0, 1.5, 0.25])])
    inner = ((g >= 4) & (g <= LATTICE_N - 5)).all(axis=1)
    return xyz, rows[0][0] + np.flatnonzero(inner)


def lattice_ball_count(steps=4):
    """Number of integer vectors v with |v|^2 < steps^2."""
    i = np.arange(-steps, steps + 1)
    v = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    return int(((v * v).sum(axis=1) < steps * steps).sum())


def one_per_cell_lattice(spacing=0.045, jitter=0.004, dims=(40, 40, 6), seed=104):
    """A jittered lattice with about one point per cell: 256 cell-ordered consecutive queries span
    far more than 64 cells (the chain consumer's per-lane run starts)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    p = 0.1 + g * spacing + rng.uniform(-jitter, jitter, (len(g), 3))
    return assemble([p])[0]


def min_cells_per_group(x, y, z, group=256):
    """Minimum, over the groups of `group` consecutive points in (x, y, z) row-major cell order, of
    the number of distinct cells in the group."""
    c = cells(np.stack([x, y, z], axis=1))
    dims = c.max(axis=0) + 1
    key = np.sort((c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2])
    return min(len(np.unique(key[i:i + group])) for i in range(0, len(key), group))


def dense_run_beside_sparse(n_sparse=100, n_dense=5000, seed=105, slot=0):
    """A blob of n_sparse points whose 3x3x3 block holds, in the z-run of the next y column, a blob
    of n_dense > 4096 points more than R away (the two-blob geometry along y and z).  The short
    lists' block has a run too long for 16-bit entries, so a compact build gives them 32-bit
    entries.  Returns the two point arrays (no anchor: for assemble())."""
    rng = np.random.default_rng(seed)
    return two_blob_pair(rng, n_sparse, n_dense, slot, axes=(1, 2))
