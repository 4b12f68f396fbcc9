"""Clouds on which the grid's cell is coarser than the search radius -- plain numpy, no GPU.

build_grid (pfx_grid.hip) starts from cell = r * (1 + 1e-6) and, while the bounding box would need
more than 2^26 cells, multiplies the cell by cbrt(total / 2^26) * 1.01.  grid_params restates that
loop; `factor` below is cell / r.  A surface patch of about 1 m (its minimum at the origin, so its
cells are known) keeps k(0.05) near 100 at 12,000 points; what is added to it decides the factor:

  compact(n)       the patch alone                                       factor 1.000001 (control)
  stray(n)         + one point at (500, 500, 500), appended last         24.85 at r = 0.05
  stray_near(n)    a patch dense towards its corner + one point at (96, 96, 96)     4.77
  two_parts(n)     two patches in a box of 30 m per axis                  1.49
  stray_inf(n)     compact + (inf, ., .) + (nan, nan, nan)               1.000001

Everything is float32 and drawn from a seeded default_rng.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

R = 0.05               # the normal radius of every test
R_FEATURE = 0.08       # FPFH with its own query cloud
R_HARRIS = 0.01
RADII = (R, R_FEATURE)
MAX_CELLS = float(1 << 26)
FAT_CAP = 1024         # kGridFatCap: the counting builder orders cells up to this many points
T_SMALL, T_SPARSE, T_DENSE = 384, 1280, 8000  # kTcapSmall / kTcapSparse / kTcapDense (candidates of a block)
STRAY = 500.0
STRAY_NEAR = 96.0
PARTS_BOX = 30.0
HARRIS_SCALE = 0.2     # two_parts at r = 0.01: the same 600 cells per axis as at r = 0.05 unscaled


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cbrt.restype = ctypes.c_double
_libm.cbrt.argtypes = [ctypes.c_double]


def _cbrt(v):
    """The C library's cbrt, which build_grid's std::cbrt is (np.cbrt differs from it by an ulp on
    these arguments, and the tests compare the cell bit for bit)."""
    return float(_libm.cbrt(float(v)))


def grid_params(lo, hi, r):
    """build_grid's cell loop: (lo, hi, r) -> (cell, dims); float64 as there."""
    lo, hi = (np.asarray(a, np.float64) for a in (lo, hi))
    cell = r * (1.0 + 1e-6)
    for _ in range(64):
        dims = [int(np.floor((hi[d] - lo[d]) / cell)) + 1 for d in range(3)]
        total = float(dims[0]) * float(dims[1]) * float(dims[2])
        if total <= MAX_CELLS:
            break
        cell *= _cbrt(total / MAX_CELLS) * 1.01
    return cell, tuple(dims)


def bounds(xyz):
    """The finite points' bounding box (float32 values, as float64)."""
    p = np.stack(xyz, axis=1)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def hint_bounds(lo, hi, r):
    """What an exact build leaves for the next speculative one: 10 % wider on every side plus 2 r."""
    lo, hi = (np.asarray(a, np.float64) for a in (lo, hi))
    m = 0.1 * (hi - lo) + 2.0 * r
    return lo - m, hi + m


def factor(xyz, r, hinted=False):
    lo, hi = bounds(xyz)
    if hinted:
        lo, hi = hint_bounds(lo, hi, r)
    return grid_params(lo, hi, r)[0] / r


def patch(n, seed, side=1.0, skew=1.0, amp=0.1):
    """A wavy, slightly noisy surface patch (n, 3) float32 with its minimum at the origin.  skew > 1
    crowds the points towards the u = v = 0 corner (u = side * t^skew, t uniform); amp is the
    wave's amplitude in sides."""
    rng = np.random.default_rng(seed)
    t = rng.random((2, n))
    u, v = (np.float32(side) * (t ** skew).astype(np.float32))
    s = np.float32(1.0 / side)
    w = (np.float32(amp * side) * np.sin(np.float32(3) * u * s) * np.cos(np.float32(2) * v * s)
         + (0.002 * side * rng.normal(size=n)).astype(np.float32)).astype(np.float32)
    p = np.stack([u, v, w], axis=1).astype(np.float32)
    return p - p.min(axis=0)


def _soa(p):
    p = np.ascontiguousarray(p, np.float32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def _seed(n):
    return 7000 + n


@functools.lru_cache(maxsize=None)
def _compact(n):
    return patch(n, _seed(n))


def compact(n):
    return _soa(_compact(n))


def stray(n):
    return _soa(np.concatenate([_compact(n), np.full((1, 3), STRAY, np.float32)]))


@functools.lru_cache(maxsize=None)
def _near_patch(n):
    return patch(n, _seed(n) + 1, skew=2.0, amp=0.25)  # (0.4 m deep: two coarse cells in z as well)


def stray_near(n):
    return _soa(np.concatenate([_near_patch(n), np.full((1, 3), STRAY_NEAR, np.float32)]))


def near_patch(n):
    """stray_near(n) without its stray: the patch's cells at factor 1 (control of the same density)."""
    return _soa(_near_patch(n))


def two_parts(n=1500, scale=1.0):
    """Two patches of n points each; the second is moved so that the box is PARTS_BOX * scale per axis."""
    a = patch(n, _seed(n) + 2, side=scale)
    b = patch(n, _seed(n) + 3, side=scale)
    b = b + (np.float32(PARTS_BOX * scale) - b.max(axis=0))
    return _soa(np.concatenate([a, b]))


def stray_inf(n):
    bad = np.array([[np.inf, 0.5, 0.1], [np.nan, np.nan, np.nan]], np.float32)
    return _soa(np.concatenate([_compact(n), bad]))


def queries(xyz, r, n_cloud=56, seed=11):
    """At most 64 queries: n_cloud points of the cloud (its last row, the stray where there is one,
    included) and eight that are no cloud points, in this order:
      0  outside the box, within r of the surface point with the smallest x;
      1  between r and one coarse cell outside the box (low x side);
      2, 3  several cells outside on the low and on the high side of every axis (clamped cells);
      4, 5  one cell + r outside on the low / high side of x alone, y and z inside;
      6  NaN;  7  +inf in y.
    Returns ((qx, qy, qz), rows) with rows[j] = the cloud row of query j or -1."""
    x, y, z = xyz
    lo, hi = bounds(xyz)
    cell, _ = grid_params(lo, hi, r)
    fin = np.flatnonzero(np.isfinite(np.stack(xyz)).all(axis=0))
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(fin[:-1], min(n_cloud - 1, len(fin) - 1), replace=False))
    pick = np.r_[pick, fin[-1]]
    i0 = fin[np.argmin(x[fin])]
    between = 0.5 * (r + cell) if cell > 1.2 * r else 1.5 * r  # (a cell of r has no such place: 1.5 r then)
    off = np.array([
        [x[i0] - 0.6 * r, y[i0], z[i0]],
        [x[i0] - between, y[i0], z[i0]],
        lo - 8.0 * cell,
        hi + 8.0 * cell,
        [lo[0] - cell - r, y[i0], z[i0]],
        [hi[0] + cell + r, y[i0], z[i0]],
        [np.nan, np.nan, np.nan],
        [x[i0], np.inf, z[i0]],
    ], np.float64).astype(np.float32)
    q = np.concatenate([np.stack([x[pick], y[pick], z[pick]], axis=1), off]).astype(np.float32)
    rows = np.r_[pick, np.full(len(off), -1)].astype(np.int64)
    return _soa(q), rows


# ---- what the grid does with a cloud, from the restated parameters --------------------------------

def cell_coords(xyz, lo, cell, dims):
    """Clamped integer cell coordinates (m, 3) of the finite points, as k_cell_keys computes them."""
    p = np.stack(xyz, axis=1)
    p = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    inv = 1.0 / cell
    c = np.floor((p - np.asarray(lo, np.float64)) * inv).astype(np.int64)
    return np.clip(c, 0, np.asarray(dims) - 1)


def cell_and_block_counts(xyz, r, hinted=False, box=None):
    """(points per occupied cell, candidates of every occupied cell's 3x3x3 block), both (cells,),
    on the grid of the cloud's own bounds or of `box` (another cloud's), exact or widened to the hint."""
    lo, hi = box if box is not None else bounds(xyz)
    if hinted:
        lo, hi = hint_bounds(lo, hi, r)
    cell, dims = grid_params(lo, hi, r)
    c = cell_coords(xyz, lo, cell, dims)
    uniq, cnt = np.unique(c, axis=0, return_counts=True)
    table = {tuple(u): int(k) for u, k in zip(uniq, cnt)}
    block = np.zeros(len(uniq), np.int64)
    for i, u in enumerate(uniq):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    block[i] += table.get((u[0] + dx, u[1] + dy, u[2] + dz), 0)
    return cnt.astype(np.int64), block


def tile_classes(xyz, r, hinted=False, box=None, tile=16):
    """Tiles (16 queries of one cell) per class implied by the block counts: dict small / sparse /
    dense / wide, as k_tile_cells classes them."""
    cnt, block = cell_and_block_counts(xyz, r, hinted, box)
    tiles = (cnt + tile - 1) // tile
    return {"small": int(tiles[block <= T_SMALL].sum()),
            "sparse": int(tiles[(block > T_SMALL) & (block <= T_SPARSE)].sum()),
            "dense": int(tiles[(block > T_SPARSE) & (block <= T_DENSE)].sum()),
            "wide": int(tiles[block > T_DENSE].sum())}


def neighbour_counts(xyz, r, chunk=256):
    """Float64 count of points within r (d2 <= r^2, the point itself included) of every finite row,
    in row order.  Every pair is tested but those more than r apart in x alone (rows are taken in x
    order, so a chunk's partners are one slice of the x-sorted points)."""
    p = np.stack(xyz, axis=1).astype(np.float64)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    order = fin[np.argsort(p[fin, 0], kind="stable")]
    ps = p[order]
    out = np.zeros(len(p), np.int64)
    for s in range(0, len(order), chunk):
        q = ps[s:s + chunk]
        a = np.searchsorted(ps[:, 0], q[0, 0] - 1.001 * r, side="left")
        b = np.searchsorted(ps[:, 0], q[-1, 0] + 1.001 * r, side="right")
        d2 = ((q[:, None, :] - ps[None, a:b, :]) ** 2).sum(axis=2)
        out[order[s:s + chunk]] = (d2 <= r * r).sum(axis=1)
    return out[fin]


ICP_DELTA = (0.02, -0.015, 0.01)


def icp_source(target, cap, step=3):
    """A source for ICP against `target` with distance cap `cap`: every step-th finite target row
    moved by -ICP_DELTA (its last row, the stray where there is one, included), then four points
    that are no shifted target rows: one outside the target's box within the cap of a target
    point, one outside beyond the cap but inside the first coarse cell, one several cells outside
    (clamped) and one NaN.  Returns (x, y, z) float32."""
    lo, hi = bounds(target)
    cell, _ = grid_params(lo, hi, cap * (1.0 + 1e-4))
    p = np.stack(target, axis=1)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    rows = np.unique(np.r_[fin[::step], fin[-1]])
    s = (p[rows] - np.asarray(ICP_DELTA, np.float32)).astype(np.float32)
    i0 = fin[np.argmin(p[fin, 0])]
    extra = np.array([p[i0] - [0.6 * cap, 0.0, 0.0], p[i0] - [0.5 * (cap + min(cell, 20 * cap)), 0.0, 0.0],
                      lo - 8.0 * cell, [np.nan, 0.0, 0.0]], np.float64).astype(np.float32)
    return _soa(np.concatenate([s, extra]))
