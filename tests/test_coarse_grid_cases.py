"""The coarse-grid clouds (coarse_grid_cases.py) are what they claim to be: the cell factor the
restated build_grid loop gives, the point counts per cell and candidate counts per 3x3x3 block
against the counting builder's and the tile classes' thresholds, the stray point's isolation and the
neighbour counts.  No GPU: nothing here asserts what the GPU code does (test_gpu_coarse_grid.py).
"""
import functools

import numpy as np
import pytest

import coarse_grid_cases as C

SIZES = (20, 3000, 12000)
NEAR = 12000


def _bytes(xyz):
    return b"".join(a.tobytes() for a in xyz)


@functools.lru_cache(maxsize=None)
def _k(case, n, r):
    return C.neighbour_counts(getattr(C, case)(n), r)


def test_restated_loop_leaves_a_fitting_box_alone_and_is_monotone():
    cell, dims = C.grid_params([0, 0, 0], [1, 1, 0.3], 0.05)
    assert cell == 0.05 * (1.0 + 1e-6) and dims == (20, 20, 6)
    # 406^3 < 2^26 < 407^3: the first box that coarsens
    assert C.grid_params([0] * 3, [405.5 * cell] * 3, 0.05)[0] == cell
    assert C.grid_params([0] * 3, [406.5 * cell] * 3, 0.05)[0] > cell
    for hi in (30.0, 96.0, 500.0, 5000.0):
        c, d = C.grid_params([0] * 3, [hi] * 3, 0.05)
        assert d[0] * d[1] * d[2] <= C.MAX_CELLS and c > 0.05


@pytest.mark.parametrize("n", SIZES)
def test_factors_of_the_patch_with_and_without_a_stray(n):
    for r in C.RADII:
        assert C.factor(C.compact(n), r) == pytest.approx(1.000001, abs=1e-9)
        assert C.factor(C.compact(n), r, hinted=True) == pytest.approx(1.000001, abs=1e-9)
        assert C.factor(C.stray_inf(n), r) == pytest.approx(1.000001, abs=1e-9)
    assert C.factor(C.stray(n), C.R) == pytest.approx(24.85, abs=0.005)
    assert C.factor(C.stray(n), C.R_FEATURE) == pytest.approx(24.85 * C.R / C.R_FEATURE, abs=0.005)
    # a hinted build's box is 20 % + 4 r wider
    assert C.factor(C.stray(n), C.R, hinted=True) == pytest.approx(29.83, abs=0.005)
    for r in C.RADII:
        lo, hi = C.bounds(C.stray(n))
        assert C.grid_params(lo, hi, r)[1] == (403, 403, 403)


def test_factors_of_stray_near_and_two_parts():
    assert 3.0 < C.factor(C.stray_near(NEAR), C.R) < 5.0
    assert C.factor(C.stray_near(NEAR), C.R) == pytest.approx(4.77, abs=0.005)
    assert C.factor(C.stray_near(NEAR), C.R_FEATURE) == pytest.approx(2.98, abs=0.005)
    assert C.factor(C.near_patch(NEAR), C.R) == pytest.approx(1.000001, abs=1e-9)
    assert C.factor(C.two_parts(), C.R) == pytest.approx(1.49, abs=0.005)
    assert C.factor(C.two_parts(), C.R, hinted=True) == pytest.approx(1.80, abs=0.005)
    # the box of 30 m fits at r = 0.08 (375^3 cells): two_parts is a coarse case at r = 0.05 only
    assert C.factor(C.two_parts(), C.R_FEATURE) == pytest.approx(1.000001, abs=1e-9)
    assert C.factor(C.two_parts(scale=C.HARRIS_SCALE), C.R_HARRIS) == pytest.approx(1.49, abs=0.005)


@pytest.mark.parametrize("n", SIZES)
def test_stray_is_the_compact_patch_plus_one_isolated_last_point(n):
    s, c = C.stray(n), C.compact(n)
    assert all(a.dtype == np.float32 for a in s + c)
    assert len(s[0]) == n + 1 and _bytes([a[:n] for a in s]) == _bytes(c)
    assert [float(a[n]) for a in s] == [C.STRAY] * 3
    assert min(float(a.min()) for a in c) == 0.0 and all(float(a.min()) == 0.0 for a in c)
    p = np.stack(s, axis=1).astype(np.float64)
    d = np.sqrt(((p[:n] - p[n]) ** 2).sum(axis=1)).min()
    assert d > 100 * max(C.RADII)
    i = C.stray_inf(n)
    assert len(i[0]) == n + 2 and _bytes([a[:n] for a in i]) == _bytes(c)
    assert np.isinf(i[0][n]) and np.isfinite(i[1][n]) and all(np.isnan(a[n + 1]) for a in i)


def test_stray_near_and_two_parts_layout():
    s = C.stray_near(NEAR)
    assert _bytes([a[:NEAR] for a in s]) == _bytes(C.near_patch(NEAR))
    p = np.stack(s, axis=1).astype(np.float64)
    assert np.sqrt(((p[:NEAR] - p[NEAR]) ** 2).sum(axis=1)).min() > 100 * max(C.RADII)
    t = C.two_parts()
    lo, hi = C.bounds(t)
    assert list(lo) == [0.0] * 3 and list(hi) == [C.PARTS_BOX] * 3 and len(t[0]) == 3000
    p = np.stack(t, axis=1).astype(np.float64)
    assert p[:1500].max() < 1.01 and p[1500:].min() > C.PARTS_BOX - 1.01  # two parts, ~29 m of nothing between


@pytest.mark.parametrize("n", SIZES)
def test_stray_cells_and_blocks(n):
    for r in C.RADII:
        cnt, blk = C.cell_and_block_counts(C.stray(n), r)
        assert sorted(cnt) == [1, n] and sorted(blk) == [1, n]  # the patch is one cell, the stray another
        lo, hi = C.bounds(C.stray(n))
        cell, dims = C.grid_params(lo, hi, r)
        c = C.cell_coords(C.stray(n), lo, cell, dims)
        assert (c[:n] == 0).all() and (c[n] == 402).all()
    if n == 20:
        assert n <= C.T_SMALL
        assert C.tile_classes(C.stray(n), C.R) == {"small": 3, "sparse": 0, "dense": 0, "wide": 0}
    if n == 3000:
        assert C.FAT_CAP < n and C.T_SPARSE < n <= C.T_DENSE
        assert C.tile_classes(C.stray(n), C.R) == {"small": 1, "sparse": 0, "dense": 188, "wide": 0}
    if n == 12000:
        assert C.FAT_CAP < n and C.T_DENSE < n
        assert C.tile_classes(C.stray(n), C.R) == {"small": 1, "sparse": 0, "dense": 0, "wide": 750}
    # on the hint of its own exact build the patch straddles a cell face or two; the fat cell stays
    cnt, blk = C.cell_and_block_counts(C.stray(n), C.R, hinted=True)
    assert len(cnt) > 2 and blk.max() == n
    assert (cnt.max() > C.FAT_CAP) == (n >= 3000)
    # ... and on the hint a compact cloud leaves, no cell is fat
    for case in (C.compact(n), C.stray_inf(n)):
        for hinted in (False, True):
            assert C.cell_and_block_counts(case, C.R, hinted)[0].max() <= C.FAT_CAP


def test_stray_near_cells_and_blocks_lie_on_both_sides_of_every_threshold():
    s = C.stray_near(NEAR)
    lo, hi = C.bounds(s)
    cell, dims = C.grid_params(lo, hi, C.R)
    c = C.cell_coords(s, lo, cell, dims)[:NEAR]
    assert list(c.max(axis=0)[:2]) == [4, 4] and c[:, 2].max() >= 1  # 5 x 5 coarse cells, 2 or more deep
    cnt, blk = C.cell_and_block_counts(s, C.R)
    assert cnt.max() > C.FAT_CAP and (cnt < C.FAT_CAP).sum() > 10
    assert blk.max() > C.T_DENSE
    assert ((blk > C.T_SPARSE) & (blk <= C.T_DENSE)).any() and ((blk > C.T_SMALL) & (blk <= C.T_SPARSE)).any()
    assert (blk <= C.T_SMALL).any()
    tc = C.tile_classes(s, C.R)
    assert all(v > 0 for v in tc.values()), tc
    assert C.cell_and_block_counts(s, C.R, hinted=True)[0].max() > C.FAT_CAP
    # without the stray the same patch has no fat cell and no wide tile
    cnt, blk = C.cell_and_block_counts(C.near_patch(NEAR), C.R)
    assert cnt.max() <= C.FAT_CAP and blk.max() <= C.T_DENSE


def test_two_parts_cells():
    for t, r in ((C.two_parts(), C.R), (C.two_parts(scale=C.HARRIS_SCALE), C.R_HARRIS)):
        cnt, blk = C.cell_and_block_counts(t, r)
        assert cnt.max() <= C.FAT_CAP and blk.max() <= C.T_SMALL
        lo, hi = C.bounds(t)
        cell, dims = C.grid_params(lo, hi, r)
        assert dims == (403, 403, 403)
        # r < cell < 2 r: along x and y every ball crosses one cell face, and some cross two
        p = np.stack(t, axis=1).astype(np.float64)
        faces = np.floor((p + r) / cell) - np.floor((p - r) / cell)
        assert set(np.unique(faces[:, :2])) == {1.0, 2.0}
        assert 0.2 < (faces[:, :2] == 2).mean() < 0.5


def test_neighbour_counts():
    """Exhaustive float64 counts: the stray has itself alone, the patch's counts are the compact
    cloud's, lists stay far below the candidates of a coarse block."""
    for n, lo_med, hi_med in ((3000, 15, 35), (12000, 80, 110)):
        ks, kc = _k("stray", n, C.R), _k("compact", n, C.R)
        assert ks[n] == 1 and np.array_equal(ks[:n], kc)
        assert kc.min() >= 1 and kc.max() <= 200 and lo_med <= np.median(kc) <= hi_med
    ks = _k("stray", 20, C.R)
    assert ks[20] == 1 and ks.max() <= 3
    kn = _k("stray_near", NEAR, C.R)
    assert kn[NEAR] == 1 and kn.min() == 1 and 512 < kn.max() <= 1024  # longest lists overflow a sparse tile only
    kt = C.neighbour_counts(C.two_parts(), C.R)
    assert kt.min() >= 1 and 10 <= kt.max() <= 40
    kh = C.neighbour_counts(C.two_parts(scale=C.HARRIS_SCALE), C.R_HARRIS)
    assert kh.min() >= 1 and 10 <= kh.max() <= 40


@pytest.mark.parametrize("case,n,r", [("stray", 12000, C.R), ("stray", 3000, C.R_FEATURE), ("stray_near", NEAR, C.R),
                                      ("two_parts", 1500, C.R), ("compact", 3000, C.R)])
def test_queries(case, n, r):
    xyz = getattr(C, case)(n)
    (qx, qy, qz), rows = C.queries(xyz, r)
    assert len(qx) <= 64 and (rows >= 0).sum() >= 16
    on = rows >= 0
    assert all(np.array_equal(q[on], a[rows[on]]) for q, a in zip((qx, qy, qz), xyz))
    fin = np.flatnonzero(np.isfinite(np.stack(xyz)).all(axis=0))
    assert rows[on][-1] == fin[-1]  # the last finite row (the stray where there is one) is a query
    lo, hi = C.bounds(xyz)
    cell, dims = C.grid_params(lo, hi, r)
    q = np.stack([qx, qy, qz], axis=1)[~on].astype(np.float64)
    p = np.stack(xyz, axis=1)[fin].astype(np.float64)
    idx = np.floor((q[:6] - lo) / cell)
    near = np.sqrt(((q[:6, None, :] - p[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    assert q[0, 0] < lo[0] and near[0] < r                       # outside the box, a neighbour inside
    assert q[1, 0] < lo[0] and r < near[1] < max(cell, 2 * r)    # outside, no neighbour, within one cell
    assert idx[1, 0] == (-1 if cell > 1.2 * r else -2)
    assert (idx[2] < -2).all() and (idx[3] > np.asarray(dims) + 1).all()  # clamped on every axis
    assert idx[4, 0] == -2 and idx[5, 0] >= dims[0] and near[4] > r and near[5] > r
    assert np.isnan(q[6]).all() and np.isinf(q[7, 1])


@pytest.mark.parametrize("case,n,cap", [("stray", 3000, 0.07), ("stray", 3000, 0.05), ("stray_near", NEAR, 0.07),
                                        ("two_parts", 1500, 0.05)])
def test_icp_source(case, n, cap):
    target = getattr(C, case)(n)
    s = np.stack(C.icp_source(target, cap), axis=1).astype(np.float64)
    t = np.stack(target, axis=1).astype(np.float64)
    lo, hi = C.bounds(target)
    cell, dims = C.grid_params(lo, hi, cap * (1.0 + 1e-4))
    assert cell > 1.4 * cap and np.isnan(s[-1, 0])
    near = np.sqrt(((s[:-1, None, :] - t[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    moved = np.linalg.norm(C.ICP_DELTA)
    assert near[:-3].max() <= moved * 1.001 < cap              # every shifted row keeps a partner within the cap
    assert np.allclose(s[-5] + C.ICP_DELTA, t[-1], atol=1e-4)  # the last shifted row is the target's last row
    assert s[-4, 0] < lo[0] and near[-3] < cap                 # outside the box, a partner within the cap
    assert s[-3, 0] < lo[0] and cap < near[-2] and np.floor((s[-3, 0] - lo[0]) / cell) == -1
    assert (np.floor((s[-2] - lo) / cell) < -2).all()          # clamped on every axis
