"""Inputs of the uniform-sampling tests (tests/test_uniform_ref.py, tests/test_gpu_uniform.py,
tests/test_uniform_facade.py) and a plain numpy statement of DESIGN.md "Uniform sampling: the
contract": lexsort by (leaf, diff, index), then the heads of the runs of equal leaf."""
import numpy as np

f32 = np.float32


def _inv(radius):
    leaf = f32(radius)
    return f32(1.0) / leaf


def cells_of(v, radius):
    """(int)floorf(v * inv): one float32 multiply, then floor."""
    return np.floor(np.asarray(v, f32) * _inv(radius)).astype(np.int64)


def diffs(x, y, z, i, j, k, scalar_order=False):
    """PCL's squared norm of (point, 1) - (cell, 0) in float32: the contract's association
    (dx^2 + dz^2) + (dy^2 + 1), or the scalar build's ((dx^2 + dy^2) + dz^2) + 1."""
    dx = np.asarray(x, f32) - i.astype(f32)
    dy = np.asarray(y, f32) - j.astype(f32)
    dz = np.asarray(z, f32) - k.astype(f32)
    if scalar_order:
        return ((dx * dx + dy * dy) + dz * dz) + f32(1.0)
    return (dx * dx + dz * dz) + (dy * dy + f32(1.0))


def numpy_statement(x, y, z, radius, scalar_order=False, plus_one=True):
    """(idx, leaf, points, cells) of a cloud whose extent an int indexes.  plus_one=False drops the
    fourth component (what a kernel that forgets it computes)."""
    x, y, z = (np.asarray(v, f32) for v in (x, y, z))
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    pts = np.flatnonzero(fin)
    if len(pts) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0
    i, j, k = (cells_of(v[pts], radius) for v in (x, y, z))
    div = [int(c.max() - c.min() + 1) for c in (i, j, k)]
    leaf = (i - i.min()) + (j - j.min()) * div[0] + (k - k.min()) * div[0] * div[1]
    d = diffs(x[pts], y[pts], z[pts], i, j, k, scalar_order)
    if not plus_one:
        dx, dy, dz = x[pts] - i.astype(f32), y[pts] - j.astype(f32), z[pts] - k.astype(f32)
        d = (dx * dx + dz * dz) + dy * dy
    order = np.lexsort((pts, d, leaf))
    sl = leaf[order]
    head = np.ones(len(order), bool)
    head[1:] = sl[1:] != sl[:-1]
    return (pts[order][head].astype(np.int32), sl[head].astype(np.int32), len(pts), div[0] * div[1] * div[2])


# ---- 1. one point per cell of a 7 x 5 x 3 lattice around the origin ---------------------------------
LATTICE_LEAF = 0.1


def lattice(seed=5):
    """Cell centres (jittered by a quarter cell) for i in [-3, 3], j in [-2, 2], k in [-1, 1], in a
    shuffled order.  Returns (x, y, z, expected idx, expected leaf)."""
    rng = np.random.default_rng(seed)
    i, j, k = (g.ravel() for g in np.meshgrid(np.arange(-3, 4), np.arange(-2, 3), np.arange(-1, 2), indexing="ij"))
    perm = rng.permutation(len(i))
    i, j, k = i[perm], j[perm], k[perm]
    jit = rng.uniform(-0.25, 0.25, (3, len(i)))
    x, y, z = (((c + 0.5 + jit[a]) * LATTICE_LEAF).astype(f32) for a, c in enumerate((i, j, k)))
    leaf = (i + 3) + (j + 2) * 7 + (k + 1) * 35
    order = np.argsort(leaf)
    return x, y, z, order.astype(np.int32), leaf[order].astype(np.int32)


# ---- 2. the +1 tie ------------------------------------------------------------------------------
#: The issue writes this case with leaf 0.5.  There the two points lie in cell (2, 2, 2), an integer
#: cell coordinate is a whole unit from each coordinate, and the diffs are 3.9996 and 3.9998: no tie.
#: At leaf 1 the same two points lie in cell (1, 1, 1), dx is 2e-4 and 1e-4, and both diffs round to
#: 1.0f, which is what the case is for.
TIE_LEAF = 1.0


def tie(swapped=False):
    """Two points of cell (1, 1, 1): the farther one first (or second, swapped).  With the fourth
    component both diffs are 1.0f, so index 0 wins either way."""
    a, b = (1 + 2e-4, 1.0, 1.0), (1 + 1e-4, 1.0, 1.0)
    rows = np.array([b, a] if swapped else [a, b], f32)
    return rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()


# ---- 3. the association -------------------------------------------------------------------------
ASSOC_LEAF = 0.5
ASSOC_CELL = (3, 2, 5)


def assoc_traded_pairs(count, seed=11):
    """Pairs of points of cell ASSOC_CELL with the same z whose x offset is traded against the y
    offset: the second point's y is solved (in float64, then rounded) so that the exact squared
    norms agree, and the float32 roundings of the sum decide the winner.  An exact swap of the two
    offsets does not exist in this cell: dx lies in [-1.5, -1) and dy in [-1, -0.5).  Returns
    (m, 2, 3) float32, m <= count (the pairs whose second point fell outside the cell are dropped).
    Measured on count = 200,000 (95,815 pairs kept): the contract's order and the scalar order pick
    different winners in 14.5 % of them."""
    rng = np.random.default_rng(seed)
    ci, cj, ck = ASSOC_CELL
    lo = np.array(ASSOC_CELL, np.float64) * ASSOC_LEAF
    xa, ya, z = (rng.uniform(lo[a], lo[a] + ASSOC_LEAF, count).astype(f32) for a in range(3))
    xb = rng.uniform(lo[0], lo[0] + ASSOC_LEAF, count).astype(f32)
    s = (xa.astype(np.float64) - ci) ** 2 + (ya.astype(np.float64) - cj) ** 2 - (xb.astype(np.float64) - ci) ** 2
    ok = s > 0
    yb = (cj - np.sqrt(np.where(ok, s, 1.0))).astype(f32)
    ok &= (yb >= f32(lo[1])) & (yb < f32(lo[1] + ASSOC_LEAF))
    return np.stack([np.stack([xa, ya, z], 1), np.stack([xb, yb, z], 1)], 1)[ok]


#: 48 pairs committed as float32 bit patterns (x0, y0, z0, x1, y1, z1), chosen by the numpy statement
#: from assoc_traded_pairs(200000): in every one the contract's order and the scalar order pick
#: different winners, 24 of each direction
ASSOC_PAIRS_BITS = (
    (0x3fc8d478, 0x3fa8ab14, 0x402dcff4, 0x3fc9314b, 0x3fa7e96b, 0x402dcff4),
    (0x3fd3c1e7, 0x3f9c4463, 0x403fe2a2, 0x3fc47538, 0x3fbd59d5, 0x403fe2a2),
    (0x3fd44fe6, 0x3fbbd043, 0x40254ce6, 0x3fd472b3, 0x3fbb78e4, 0x40254ce6),
    (0x3fc3e591, 0x3f9caab6, 0x4025386e, 0x3fce33d7, 0x3f8b37e4, 0x4025386e),
    (0x3fced392, 0x3f8aad07, 0x402c881b, 0x3fc2792e, 0x3f9fe697, 0x402c881b),
    (0x3fd24ae9, 0x3fbc9a5c, 0x4036ea08, 0x3fe02094, 0x3fa04e5d, 0x4036ea08),
    (0x3ff366d8, 0x3f9f1a93, 0x4039b407, 0x3ffaf286, 0x3f94fa55, 0x4039b407),
    (0x3ff80b7a, 0x3f824cb0, 0x403a5028, 0x3fdc7d92, 0x3fa91d5d, 0x403a5028),
    (0x3fe7a327, 0x3f85aec9, 0x4037b6e1, 0x3fcd5ad9, 0x3fb0de4d, 0x4037b6e1),
    (0x3fe2a829, 0x3f9c223f, 0x403cca7e, 0x3fdd01b1, 0x3fa5a62f, 0x403cca7e),
    (0x3fd26df0, 0x3fa40dd2, 0x403ef7e9, 0x3fea3a73, 0x3f80eb99, 0x403ef7e9),
    (0x3ff7fd8e, 0x3f8aedcb, 0x403a29e9, 0x3fdf2e60, 0x3fb05dbf, 0x403a29e9),
    (0x3ff3c9ee, 0x3f8103e1, 0x4036933d, 0x3feef5ce, 0x3f868f3e, 0x4036933d),
    (0x3ff9c26c, 0x3fbbde41, 0x403829b4, 0x3ffb3ba5, 0x3fb90a1f, 0x403829b4),
    (0x3ffded53, 0x3f9690fa, 0x40338ce1, 0x3ffb2244, 0x3f9a1bd9, 0x40338ce1),
    (0x3fcaa13a, 0x3faf2196, 0x4021d4c5, 0x3fe54d1b, 0x3f837cf9, 0x4021d4c5),
    (0x3fde9142, 0x3fbab75b, 0x4039c39a, 0x3ffd2437, 0x3f8acbca, 0x4039c39a),
    (0x3fd99220, 0x3fbe9d48, 0x40385e14, 0x3ff5cf93, 0x3f8e851e, 0x40385e14),
    (0x3fe64ee5, 0x3f8820cb, 0x403a232e, 0x3fd263be, 0x3fa76683, 0x403a232e),
    (0x3fe4152d, 0x3f98add3, 0x40290e95, 0x3ff18010, 0x3f86d791, 0x40290e95),
    (0x3fd44d9c, 0x3f8f27f5, 0x40200bea, 0x3fc38b11, 0x3fae2940, 0x40200bea),
    (0x3fd9f037, 0x3f85f7d1, 0x40304207, 0x3fd563f3, 0x3f8c6967, 0x40304207),
    (0x3fd396ad, 0x3fada7d5, 0x403eaa87, 0x3fe440b3, 0x3f91530c, 0x403eaa87),
    (0x3fd5f84d, 0x3fb3b208, 0x4023b2db, 0x3fe46726, 0x3f996c23, 0x4023b2db),
    (0x3ff3371e, 0x3f886ebd, 0x40277eae, 0x3fe27c61, 0x3f9f884c, 0x40277eae),
    (0x3fe10a0e, 0x3fa1e511, 0x403f53cc, 0x3feb59cf, 0x3f92543b, 0x403f53cc),
    (0x3fd4b36f, 0x3f935531, 0x4037e6d3, 0x3fd77d0c, 0x3f8f0ef3, 0x4037e6d3),
    (0x3fd7d30a, 0x3f90ce33, 0x403f5808, 0x3fd7245d, 0x3f91d82a, 0x403f5808),
    (0x3fed5de8, 0x3f811f60, 0x4034b7a1, 0x3fdee792, 0x3f9413a3, 0x4034b7a1),
    (0x3fe360ac, 0x3f9aa4f1, 0x403e9671, 0x3fdacf80, 0x3fa94e21, 0x403e9671),
    (0x3fe622d3, 0x3fb0fea8, 0x40332ab5, 0x3ffbfc59, 0x3f903fdd, 0x40332ab5),
    (0x3fe68bf4, 0x3fb87c85, 0x403e983c, 0x3feaaae0, 0x3fb03d09, 0x403e983c),
    (0x3fd261bc, 0x3fb5c7fa, 0x40337b7e, 0x3fe0eff9, 0x3f9a42d5, 0x40337b7e),
    (0x3fe90fa2, 0x3f95731e, 0x40264b80, 0x3fe15f13, 0x3fa146d9, 0x40264b80),
    (0x3fc5b2e7, 0x3fafd77e, 0x40371209, 0x3fc0a752, 0x3fbcc4d8, 0x40371209),
    (0x3fe9a737, 0x3fb5d8dd, 0x40222387, 0x3feb9f5f, 0x3fb1fb2b, 0x40222387),
    (0x3fffc129, 0x3f854fd8, 0x40356dde, 0x3febe27e, 0x3f9e380b, 0x40356dde),
    (0x3fcf85c1, 0x3fa3a0d2, 0x402b1fe6, 0x3fdaadff, 0x3f90e320, 0x402b1fe6),
    (0x3fe26e26, 0x3fbe3455, 0x403c5e29, 0x3fff8a9b, 0x3f8f80a8, 0x403c5e29),
    (0x3fdc2734, 0x3fa853ec, 0x403cc736, 0x3ff0159b, 0x3f8a707a, 0x403cc736),
    (0x3fe71ac4, 0x3fa25c40, 0x403974e2, 0x3fda4aba, 0x3fbb8b42, 0x403974e2),
    (0x3fda6d7d, 0x3fa1cd40, 0x402f2ef3, 0x3feb8c18, 0x3f88a132, 0x402f2ef3),
    (0x3fcb29d3, 0x3fba45f3, 0x403c276e, 0x3fd9c9e1, 0x3f9c5029, 0x403c276e),
    (0x3fe361a4, 0x3fb8e008, 0x403d02b6, 0x3feaa1e7, 0x3faab125, 0x403d02b6),
    (0x3fdcfca3, 0x3fb302f2, 0x402f4160, 0x3fe3695b, 0x3fa6aa7e, 0x402f4160),
    (0x3fd49089, 0x3f8d887a, 0x40390608, 0x3fc10531, 0x3fb26a1b, 0x40390608),
    (0x3fdb1ab9, 0x3f8ec65b, 0x40327ca8, 0x3fd1d701, 0x3f9d9e8f, 0x40327ca8),
    (0x3fd3d27b, 0x3fad05e8, 0x402e3b78, 0x3ff14b09, 0x3f80dba0, 0x402e3b78),
)


def assoc_pairs():
    """ASSOC_PAIRS_BITS as (48, 2, 3) float32."""
    return np.array(ASSOC_PAIRS_BITS, np.uint32).view(f32).reshape(-1, 2, 3)


def assoc_winner(pairs, scalar_order):
    """The winner (0 or 1) of every pair taken as its own two-point cloud; -1 where the points do
    not share a cell."""
    x, y, z = pairs[..., 0], pairs[..., 1], pairs[..., 2]
    i, j, k = (cells_of(v, ASSOC_LEAF) for v in (x, y, z))
    same = (i[:, 0] == i[:, 1]) & (j[:, 0] == j[:, 1]) & (k[:, 0] == k[:, 1])
    d = diffs(x, y, z, i, j, k, scalar_order)
    return np.where(same, (d[:, 1] < d[:, 0]).astype(np.int64), -1)


# ---- 4. cell edges ------------------------------------------------------------------------------
EDGE_LEAVES = (0.05, 0.01, 0.08)


def cell_edges(leaf):
    """x = (float)(k leaf) for k in [-2000, 2000), y = z = 0: points on (or a rounding off) the
    cell boundaries.  Returns (x, y, z, k)."""
    k = np.arange(-2000, 2000)
    x = (k * float(leaf)).astype(f32)
    return x, np.zeros_like(x), np.zeros_like(x), k


# ---- 5. the synthetic room ----------------------------------------------------------------------
ROOM_N = 20000
ROOM_LEAVES = (0.05, 0.02)


def room(n=ROOM_N, seed=1):
    from pcl_feature_extraction_amd.synth import synth_room
    x, y, z, _ = synth_room(n, seed)
    return x, y, z


# ---- GPU cases beyond these ---------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 257, 1025)


def one_cell(n=5000, dup=100, seed=3):
    """n points of one cell at leaf 1.0, `dup` of them exact copies of earlier points (ties that the
    index decides), in a run longer than a workgroup."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, (n, 3)).astype(f32) + f32(4.0)
    src = rng.choice(n - dup, dup, replace=False)
    dst = rng.choice(np.arange(n - dup, n), dup, replace=False)
    p[dst] = p[src]
    # the smallest diff twice: the copy sits before the original's copy target, the index decides
    d = diffs(p[:, 0], p[:, 1], p[:, 2], *(cells_of(p[:, a], 1.0) for a in range(3)))
    best = int(np.argmin(d))
    p[n - 1] = p[best]
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def clumps(seed=4):
    """Twelve points in two clumps 1,000 m apart along x (leaf 0.01: 100,001 cells along x)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 0.0099, (12, 3))
    p[6:, 0] += 1000.0
    p = p.astype(f32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def cube_corners(edge):
    """The eight corners of a cube of that edge, centred at the origin."""
    h = edge / 2.0
    p = np.array([[sx * h, sy * h, sz * h] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], f32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def room_with_nonfinite(seed=6):
    """The room with NaN, +inf and -inf in each coordinate of rows scattered through it.  Returns
    (x, y, z, the rows' indices)."""
    x, y, z = (v.copy() for v in room())
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(x), 90, replace=False)
    bad = (np.nan, np.inf, -np.inf)
    for m, r in enumerate(rows):
        (x, y, z)[m % 3][r] = bad[(m // 3) % 3]
    # a non-finite row's other coordinates must not widen the bounds either
    x[rows[1]], z[rows[1]] = 1e6, -1e6
    return x, y, z, np.sort(rows)
