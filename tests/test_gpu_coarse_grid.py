"""The grid and its first consumers where the cell is coarser than the search radius (pfx_grid.hip
build_grid's cell loop; clouds and the restated loop in coarse_grid_cases.py, their properties in
test_coarse_grid_cases.py).

  * the path is taken: Context.grid_debug returns the restated loop's cell and dimensions, and
    perm / skeys / cell_start equal NumPy's for the exact build, a hinted radix build and a hinted
    counting build, whose fat bit and exact rerun follow from the CPU-side cell counts; the normal
    estimation's tile classes are those the candidate counts imply;
  * parity, every comparison the operation's own GPU test makes (raw bits against the CPU
    restatement): normals through the host call, normals_dev, the launch / finish pair and
    normals_fast (its own bar: the oracle's NaN pattern and the angle bounds), radius_search, FPFH
    (same_as_surface true and false, the prepared path, the support-mask path), SHOT-352 and its LRF;
  * a stray point leaves every other row's bits alone (normals, radius_search, FPFH, SHOT at 12,000);
  * compact and stray scans in turn on one Context: reruns as the hint implies, oracle bits each time.

Descriptors, keypoints and the operations left out: test_gpu_coarse_grid_descriptors.py.
"""
import functools

import numpy as np
import pytest

import coarse_grid_cases as C
import oracle_lib as O
from parity import bits, bits_equal
from pcl_feature_extraction_amd import Context, PfxError
from test_gpu_fpfh_prepared import R as R_PREPARED, _run as fpfh_prepared_run
from test_gpu_fpfh_support import R as R_SUPPORT, _pipeline_call as fpfh_pipeline_call
from test_gpu_gridbuild import FAT_BIT, _check as check_grid_arrays, _same_grid
from test_gpu_shot import _check as check_shot
from test_gpu_tile_setup import STATS as TILE_STATS

pytestmark = pytest.mark.gpu

CASES = {
    "stray(20)": (lambda: C.stray(20), C.R),
    "stray(3000)": (lambda: C.stray(3000), C.R),
    "stray(3000) at 0.08": (lambda: C.stray(3000), C.R_FEATURE),
    "stray(12000)": (lambda: C.stray(12000), C.R),
    "stray_near(12000)": (lambda: C.stray_near(12000), C.R),
    "two_parts": (lambda: C.two_parts(), C.R),
    "two_parts for Harris": (lambda: C.two_parts(scale=C.HARRIS_SCALE), C.R_HARRIS),
    "stray_inf(3000)": (lambda: C.stray_inf(3000), C.R),
    "compact(3000)": (lambda: C.compact(3000), C.R),
}
COARSE = [k for k in CASES if not k.startswith(("stray_inf", "compact"))]
NORMAL_CASES = ["stray(20)", "stray(3000)", "stray(12000)", "stray_near(12000)", "two_parts", "stray_inf(3000)"]


def _case(name):
    make, r = CASES[name]
    return make(), r


COUNTERS = ("grid_fat_fallbacks", "normals_speculative_reruns", "fpfh_speculative_reruns")


def _stat(c, name):
    """A counter that exists only from the first time its code ran: 0 until then.  Only these three
    names, and only the library's "unknown stat" error: anything else is raised."""
    assert name in COUNTERS, name
    try:
        return c.stat(name)
    except PfxError as e:
        if "unknown stat " + name not in str(e):
            raise
        return 0


@functools.lru_cache(maxsize=None)
def _normals_ref(name):
    xyz, r = _case(name)
    return O.normals(*xyz, r)


def _same_normals(got, want, what):
    for a, b in zip(got, want):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        assert bits_equal(a, b), what


def _tile_classes_seen(c):
    return {"small": c.stat("normals_tiles_small"), "sparse": c.stat("normals_tiles_sparse"),
            "dense": c.stat("normals_tiles_dense"), "wide": c.stat("normals_wide")}


def _dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in arrs]


def _outs(n, k=4):
    import torch
    t = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(k)]
    torch.cuda.synchronize()  # (a context runs on its own stream)
    return t


# ---- the path is taken ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_grid_is_the_restated_loops(monkeypatch, name):
    xyz, r = _case(name)
    lo, hi = C.bounds(xyz)
    cell, dims = C.grid_params(lo, hi, r)
    hlo, hhi = C.hint_bounds(lo, hi, r)
    hcell, hdims = C.grid_params(hlo, hhi, r)
    assert (cell > 1.4 * r) == (name in COARSE) and hcell >= cell
    fat = bool(C.cell_and_block_counts(xyz, r, hinted=True)[0].max() > C.FAT_CAP)

    def params(g):
        return (1.0 / g["inv"], (g["nx"], g["ny"], g["nz"]), (g["ox"], g["oy"], g["oz"]))

    def hinted(c, builder):
        monkeypatch.setenv("PFX_GRID_BUILD", builder)
        g = c.grid_debug(*xyz, r, mode=1)
        monkeypatch.delenv("PFX_GRID_BUILD")
        return check_grid_arrays(g, xyz, f"{name}: hinted {builder}")

    with Context(0) as c:
        g0 = check_grid_arrays(c.grid_debug(*xyz, r, mode=0), xyz, name + ": exact")
        assert g0["cap"] == C.FAT_CAP
        assert g0["inv"] == 1.0 / cell and params(g0)[1:] == (dims, tuple(lo))
        assert g0["builder"] == "sort" and not g0["rerun"]
        print(name, "cell / r", params(g0)[0] / r, dims, "hinted", hcell / r, hdims, "fat cell on the hint", fat)
        gs = hinted(c, "sort")
        assert gs["inv"] == 1.0 / hcell and params(gs)[1:] == (hdims, tuple(hlo))
        assert gs["builder"] == "sort" and gs["word"] == 0 and not gs["rerun"]
        fallbacks = _stat(c, "grid_fat_fallbacks")
        gc = hinted(c, "count")
        assert gc["builder"] == "count"
        if fat:  # a cell over the cap: the fat bit alone (no point outside), then the exact build
            assert gc["word"] == FAT_BIT and gc["rerun"]
            _same_grid(gc, g0, name + ": exact rerun of the counting build")
            assert _stat(c, "grid_fat_fallbacks") == fallbacks + 1
            again = check_grid_arrays(c.grid_debug(*xyz, r, mode=1), xyz, name + ": after the fat cell")
            assert again["builder"] == "sort" and again["word"] == 0  # the grid remembers: radix from now on
            assert _stat(c, "grid_fat_fallbacks") == fallbacks + 1
        else:
            assert gc["word"] == 0 and not gc["rerun"]
            _same_grid(gc, gs, name + ": counting build vs radix build")
            assert _stat(c, "grid_fat_fallbacks") == fallbacks


@pytest.mark.parametrize("name", NORMAL_CASES)
def test_normals_and_tile_classes(name):
    """Context.normals on a fresh context builds on exact bounds: the tile statistics are those of
    the restated grid's candidate counts (a wide tile for every tile of stray(12000)).  The second
    call builds on the hint.  An exact build of a grid that has speculative users also says whether
    a cell is over the counting builder's cap (k_fat_cells); the hinted build then takes the radix
    builder, so no fat-cell fallback happens here (test_normals_call_order reaches that one): no
    rerun, and the classes are the hinted grid's."""
    xyz, r = _case(name)
    want = _normals_ref(name)
    finite = int(np.isfinite(np.stack(xyz)).all(axis=0).sum())
    classes = {h: C.tile_classes(xyz, r, hinted=h) for h in (False, True)}
    fat_exact, fat_hint = (bool(C.cell_and_block_counts(xyz, r, hinted=h)[0].max() > C.FAT_CAP) for h in (False, True))
    assert fat_exact or not fat_hint  # (no case here whose hinted grid alone has a fat cell)

    def seen(c):
        return _tile_classes_seen(c), {k: c.stat(k) for k in TILE_STATS}

    with Context(0) as c:
        _same_normals(c.normals(*xyz, r), want, name + ": first call")
        got, s = seen(c)
        print(name, "exact", s, "fat fallbacks", _stat(c, "grid_fat_fallbacks"))
        assert got == classes[False] and s["normals_queries"] == finite
        if name == "stray(12000)":
            assert got["wide"] == 750 and got["dense"] == got["sparse"] == 0
        reruns, fallbacks = _stat(c, "normals_speculative_reruns"), _stat(c, "grid_fat_fallbacks")
        _same_normals(c.normals(*xyz, r), want, name + ": second call")
        got, s = seen(c)
        print(name, "hinted", s, "reruns", _stat(c, "normals_speculative_reruns") - reruns, "fat fallbacks",
              _stat(c, "grid_fat_fallbacks") - fallbacks)
        assert _stat(c, "grid_fat_fallbacks") == fallbacks
        assert _stat(c, "normals_speculative_reruns") == reruns
        assert got == classes[True]
        _same_normals(c.normals(*xyz, r), want, name + ": third call")


@pytest.mark.parametrize("name", NORMAL_CASES)
def test_normals_device_entry_points(name):
    import torch
    xyz, r = _case(name)
    want = _normals_ref(name)
    n = len(xyz[0])
    d = _dev(*xyz)
    with Context(0) as c:
        for call in range(3):  # exact bounds, the hint (counting builder), the hint again
            o = _outs(n)
            c.normals_dev(*d, r, *o)
            c.synchronize()
            _same_normals(o, want, f"{name}: normals_dev call {call}")
    with Context(0) as c:
        for call in range(3):
            o = _outs(n)
            c.normals_launch_dev(*d, r, *o)
            rerun = c.normals_finish_dev()
            c.synchronize()
            torch.cuda.synchronize()
            print(name, "launch / finish call", call, "rerun", rerun)
            _same_normals(o, want, f"{name}: launch / finish call {call}")
    with Context(0) as c:  # the two-phase form: lists, then chains
        o = _outs(n)
        c.normals_lists_dev(*d, r, *o)
        c.normals_chains_dev(c, *o)
        c.synchronize()
        _same_normals(o, want, name + ": lists + chains")


@pytest.mark.parametrize("name", ["stray(3000)", "stray(12000)", "stray_near(12000)", "two_parts"])
def test_normals_fast(ctx, name):
    """test_gpu_normals_fast.py's bars.  Everywhere: the oracle's NaN pattern exactly (the
    neighbour set is FLANN's).  On the patches at the origin: the angle to the PCL-order normals
    median < 0.5 deg and p99 < 5 deg, the curvature's median relative deviation < 5 %.  Half of
    two_parts lies 30 m from the origin, where PCL's single-pass float covariance of raw
    coordinates is itself degrees off (the fast path centres its sums), so there the other bar of
    that file applies to the whole cloud: against a float64 two-pass covariance over FLANN's
    neighbours the fast normals are at least as accurate as the PCL-order ones, in the median and at
    p99; the angle and curvature bars are applied to its first part, which lies at the origin."""
    from test_gpu_normals_fast import _angles, _truth
    xyz, r = _case(name)
    ox, oy, oz, oc = _normals_ref(name)
    ok = ~np.isnan(ox)
    if name == "two_parts":
        rows = np.flatnonzero(ok)
        truth = _truth(*xyz, rows, r, cap=64)
        assert not np.isnan(truth).any()
        e_pcl = _angles(np.stack([ox, oy, oz], 1)[rows], truth)
    for form in ("host", "dev"):
        if form == "host":
            fx, fy, fz, fc = ctx.normals_fast(*xyz, r)
        else:
            o = _outs(len(xyz[0]))
            ctx.normals_fast_dev(*_dev(*xyz), r, *o)
            ctx.synchronize()
            fx, fy, fz, fc = (t.cpu().numpy() for t in o)
        assert np.array_equal(np.isnan(fx), np.isnan(ox)), form
        fast = np.stack([fx, fy, fz], 1)[ok]
        ang = _angles(fast, np.stack([ox, oy, oz], 1)[ok])
        print(name, form, "angle to the PCL-order normals: median", np.median(ang), "p99", np.percentile(ang, 99))
        if name == "two_parts":
            e_fast = _angles(fast, truth)
            print(name, form, "angle to the float64 truth: fast median", np.median(e_fast), "p99", np.percentile(e_fast, 99),
                  "PCL order median", np.median(e_pcl), "p99", np.percentile(e_pcl, 99))
            assert np.median(e_fast) <= np.median(e_pcl)
            assert np.percentile(e_fast, 99) <= np.percentile(e_pcl, 99) + 1e-3
        bar = ok & (np.arange(len(ox)) < 1500) if name == "two_parts" else ok  # (the part at the origin)
        ang = _angles(np.stack([fx, fy, fz], 1)[bar], np.stack([ox, oy, oz], 1)[bar])
        rel = np.abs(fc[bar] - oc[bar]) / np.maximum(np.abs(oc[bar]), 1e-6)
        print(name, form, "where the bars apply: angle median", np.median(ang), "p99", np.percentile(ang, 99),
              "curvature median deviation", np.median(rel))
        assert np.median(ang) < 0.5 and np.percentile(ang, 99) < 5.0
        assert np.median(rel) < 0.05


# ---- radius search ----------------------------------------------------------------------------------

def _check_search(got, want, cap):
    assert np.array_equal(got[0], want[0])
    for j, k in enumerate(np.minimum(want[0], cap)):
        assert np.array_equal(got[1][j, :k], want[1][j, :k]), j
        assert np.array_equal(bits(got[2][j, :k]), bits(want[2][j, :k])), j


@pytest.mark.parametrize("name", COARSE)
def test_radius_search(ctx, name):
    """Counts, indices and d2 bits for cloud rows and for the queries that are no cloud points:
    outside the box with and without a neighbour, a coarse cell away, clamped on every side, NaN,
    inf (coarse_grid_cases.queries)."""
    xyz, r = _case(name)
    q, rows = C.queries(xyz, r)
    cap = 1024
    want = O.radius_search(*xyz, *q, r, cap=cap)
    off = want[0][rows < 0]
    assert off[0] >= 1 and (off[1:] == 0).all() and want[0][rows >= 0].min() >= 1 and want[0].max() <= cap
    _check_search(ctx.radius_search(*xyz, *q, r, cap=cap), want, cap)
    assert np.array_equal(ctx.radius_search(*xyz, *q, r)[0], want[0])  # counts only


# ---- FPFH and SHOT ----------------------------------------------------------------------------------

FEATURE_CASES = [("stray(3000)", C.R), ("stray(3000)", C.R_FEATURE), ("stray(12000)", C.R),
                 ("stray_near(12000)", C.R), ("two_parts", C.R)]


@functools.lru_cache(maxsize=None)
def _feature_case(name, r):
    """(cloud, oracle normals at 0.05, queries at r, their cloud rows)."""
    xyz, _ = _case(name)
    q, rows = C.queries(xyz, r)
    return xyz, _normals_ref(name)[:3], q, rows


def _rows_differ(got, want):
    return np.flatnonzero((bits(got) != bits(want)).any(axis=1))


@pytest.mark.parametrize("name,r", FEATURE_CASES)
def test_fpfh_with_its_own_queries(ctx, name, r):
    xyz, nrm, q, rows = _feature_case(name, r)
    want = O.fpfh(*xyz, *nrm, *q, r)
    assert np.isnan(want[rows < 0][1:]).all() and not np.isnan(want[rows >= 0][:-1]).any()
    got = ctx.fpfh(*xyz, *nrm, *q, r)
    bad = _rows_differ(got, want)
    assert got.shape == want.shape and len(bad) == 0, f"rows {bad[:8].tolist()} differ from the oracle"


@pytest.mark.parametrize("name", ["stray(3000)", "stray_near(12000)", "two_parts"])
def test_fpfh_same_as_surface(ctx, name):
    xyz, r = _case(name)
    nrm = _normals_ref(name)[:3]
    want = O.fpfh(*xyz, *nrm, *xyz, r, same_as_surface=True, threads=8)
    got = ctx.fpfh(*xyz, *nrm, None, None, None, r, same_as_surface=True)
    bad = _rows_differ(got, want)
    assert got.shape == want.shape and len(bad) == 0, f"rows {bad[:8].tolist()} differ from the oracle"


@pytest.mark.parametrize("name", ["stray(12000)", "stray_near(12000)", "two_parts"])
def test_fpfh_prepared_and_support_mask_paths(name):
    """test_gpu_fpfh_prepared.py's fpfh_dev with and without prepared queries, and
    test_gpu_fpfh_support.py's pipeline call (grid, S and keys prepared, the 2 r support mask handed
    over), twice on one context: exact bounds, then the hint."""
    import torch
    assert R_PREPARED == R_SUPPORT == C.R
    xyz, nrm, q, rows = _feature_case(name, C.R)
    want = O.fpfh(*xyz, *nrm, *q, C.R)
    s, n, qd = _dev(*xyz), _dev(*nrm), _dev(*q)
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        plain, used = fpfh_prepared_run(c, s, n, qd)
        assert used == 0
        prep, used = fpfh_prepared_run(c, s, n, qd, prepare_for=qd)
        assert used == 1
    p = np.stack(xyz, axis=1)
    qa = np.stack(q, axis=1)
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        first = fpfh_pipeline_call(c, p, nrm, qa)
        reruns = _stat(c, "fpfh_speculative_reruns")
        second = fpfh_pipeline_call(c, p, nrm, qa)
        assert _stat(c, "fpfh_speculative_reruns") == reruns  # every point is inside its own hint
    for what, got in (("unprepared", plain), ("prepared", prep), ("pipeline call", first), ("pipeline call, hinted", second)):
        bad = _rows_differ(got, want)
        assert len(bad) == 0, f"{name} {what}: rows {bad[:8].tolist()} of {len(want)} differ from the oracle"


@pytest.mark.parametrize("name,r", FEATURE_CASES)
def test_shot_and_its_frame(ctx, name, r):
    xyz, nrm, q, rows = _feature_case(name, r)
    want = O.shot(*xyz, *nrm, *q, r)
    valid = check_shot(ctx.shot(*xyz, *nrm, *q, r), want)
    assert valid >= (20 if name != "two_parts" else 5) and np.isnan(want[0][rows < 0][1:]).all()
    frames = ctx.shot_lrf(*xyz, *q, r)
    ok = ~np.isnan(want[0]).any(axis=1)
    assert np.array_equal(bits(frames[ok]), bits(want[1][ok]))


# ---- a stray point changes no other row -----------------------------------------------------------------

def test_stray_point_leaves_the_patch_rows_alone(ctx):
    n = 12000
    s, c = C.stray(n), C.compact(n)
    r = C.R
    ns, nc = ctx.normals(*s, r), ctx.normals(*c, r)
    for a, b in zip(ns, nc):
        assert bits_equal(a[:n], b) and np.isnan(a[n])  # one neighbour: no normal
    for form in ("host", "dev"):
        outs = []
        for xyz in (s, c):
            if form == "host":
                outs.append(ctx.normals_fast(*xyz, r))
            else:
                o = _outs(len(xyz[0]))
                ctx.normals_fast_dev(*_dev(*xyz), r, *o)
                ctx.synchronize()
                outs.append([t.cpu().numpy() for t in o])
        # normals_fast sums each point's neighbours in the grid's cell order, 16 consecutive grid
        # points centred on the first of them (pfx_normals_fast.hip); the stray's grid has other cells,
        # so another order and other centres: the neighbour sets are equal, the float sums are not
        # bit for bit.  What is invariant is compared: who has a normal.
        for a, b in zip(*outs):
            assert np.array_equal(np.isnan(a[:n]), np.isnan(b)) and np.isnan(a[n])
    cap = 256
    cs, isx, ds = ctx.radius_search(*s, *s, r, cap=cap)
    cc, icx, dc = ctx.radius_search(*c, *c, r, cap=cap)
    assert cc.max() <= cap and np.array_equal(cs[:n], cc) and cs[n] == 1
    assert isx[n, 0] == n and ds[n, 0] == 0.0
    for j in range(n):
        k = cc[j]
        assert np.array_equal(isx[j, :k], icx[j, :k]) and np.array_equal(bits(ds[j, :k]), bits(dc[j, :k])), j
    nrm = nc[:3]
    nrm_s = [np.r_[a, np.float32(np.nan)].astype(np.float32) for a in nrm]
    fs = ctx.fpfh(*s, *nrm_s, None, None, None, r, same_as_surface=True)
    fc = ctx.fpfh(*c, *nrm, None, None, None, r, same_as_surface=True)
    assert bits_equal(fs[:n], fc)
    q = tuple(a[::200].copy() for a in c)
    qs = tuple(np.r_[a, np.float32(C.STRAY)].astype(np.float32) for a in q)
    fs, fc = ctx.fpfh(*s, *nrm_s, *qs, C.R_FEATURE), ctx.fpfh(*c, *nrm, *q, C.R_FEATURE)
    assert bits_equal(fs[:-1], fc) and not np.isnan(fc).any()
    ss, sc = ctx.shot(*s, *nrm_s, *qs, C.R_FEATURE), ctx.shot(*c, *nrm, *q, C.R_FEATURE)
    assert bits_equal(ss[0][:-1], sc[0]) and bits_equal(ss[1][:-1], sc[1]) and not np.isnan(sc[0]).any()
    assert np.isnan(ss[0][-1]).all()  # fewer than 5 neighbours: no descriptor
    # the stray's own rows are those of a cloud of one point
    one = tuple(np.array([C.STRAY], np.float32) for _ in range(3))
    nan1 = [np.array([np.nan], np.float32)] * 3
    assert bits_equal(fs[-1:], ctx.fpfh(*one, *nan1, *one, C.R_FEATURE))
    assert bits_equal(ss[0][-1:], ctx.shot(*one, *nan1, *one, C.R_FEATURE)[0])


# ---- compact and stray scans in turn on one context ---------------------------------------------------

@pytest.mark.parametrize("n", [3000, 12000])
def test_normals_call_order(n):
    """(speculative reruns, fat-cell fallbacks) of every call, as the hints and the CPU-side cell
    counts imply them, and the oracle's bits each time.

    compact, compact, stray, compact, compact: the stray lies outside the compact hint (one rerun on
    exact bounds, which finds the stray grid's fat cell); the compact scans after it lie inside the
    stray's hint and are built on its coarse cells by the radix builder (the fat cell is known): no
    rerun, no exact build, so the hint stays coarse.

    stray(20), compact(n), compact(n): the exact build of stray(20) has no fat cell, so compact(n)
    takes the counting builder on a hint whose cells hold more than 1024 of its points: the fat bit,
    one rerun on exact bounds, which shrinks the hint back; the next call is an ordinary hinted one."""
    s, c, s20 = C.stray(n), C.compact(n), C.stray(20)
    want_s, want_c = O.normals(*s, C.R), O.normals(*c, C.R)
    lo, hi = C.hint_bounds(*C.bounds(s20), C.R)
    cell, dims = C.grid_params(lo, hi, C.R)
    cnt = np.unique(C.cell_coords(c, lo, cell, dims), axis=0, return_counts=True)[1]
    assert cell > 20 * C.R and cnt.max() > C.FAT_CAP and C.neighbour_counts(s20, C.R).max() <= 3
    assert (lo < C.bounds(c)[0]).all() and (hi > C.bounds(c)[1]).all()

    def run(ctx, xyz, want, what):
        before = (_stat(ctx, "normals_speculative_reruns"), _stat(ctx, "grid_fat_fallbacks"))
        got = ctx.normals(*xyz, C.R)
        _same_normals(got, want, what)
        return _stat(ctx, "normals_speculative_reruns") - before[0], _stat(ctx, "grid_fat_fallbacks") - before[1]

    with Context(0) as fresh:
        fresh_c = fresh.normals(*c, C.R)
    _same_normals(fresh_c, want_c, "fresh context")
    with Context(0) as ctx:
        seen = [run(ctx, xyz, want, f"call {i}") for i, (xyz, want) in
                enumerate([(c, want_c), (c, want_c), (s, want_s), (c, want_c), (c, want_c)])]
        print("normals call order", n, seen)
        assert seen[0][0] in (0, 1) and seen[0][1] == 0  # exact bounds (a fresh list buffer may be short)
        assert seen[1:] == [(0, 0), (1, 0), (0, 0), (0, 0)]
        on_stray_hint = C.tile_classes(c, C.R, hinted=True, box=C.bounds(s))
        assert _tile_classes_seen(ctx) == on_stray_hint and on_stray_hint["wide" if n == 12000 else "dense"] > 100
    with Context(0) as ctx:
        seen = [run(ctx, s20, O.normals(*s20, C.R), "stray(20)"), run(ctx, c, want_c, "compact on the coarse hint"),
                run(ctx, c, want_c, "compact again")]
        print("normals call order after stray(20)", n, seen)
        assert seen[0][0] in (0, 1) and seen[0][1] == 0
        assert seen[1:] == [(1, 1), (0, 0)]
        assert _tile_classes_seen(ctx) == C.tile_classes(c, C.R, hinted=True)


def test_fpfh_call_order():
    """test_fpfh_speculative_surface_grid's sequence (prepare, normals, prepared queries, fpfh_dev)
    on compact, compact, stray, compact, compact: the stray scan lies outside the hint (one rerun);
    the compact scan after it is inside the coarse hint (no rerun: a prepared grid comes from the
    radix builder or is validated as a whole); every result equals the host call's on a fresh context."""
    import torch
    n = 3000
    s, c = C.stray(n), C.compact(n)
    dev = torch.device("cuda", 0)
    seen = []
    with Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        for i, xyz in enumerate((c, c, s, c, c)):
            q, rows = C.queries(xyz, C.R_FEATURE)
            t, qs = _dev(*xyz), _dev(*q)
            nrm = [torch.empty_like(t[0]) for _ in range(4)]
            out = torch.empty((len(q[0]), 33), dtype=torch.float32, device=dev)
            before = _stat(ctx, "fpfh_speculative_reruns")
            ctx.fpfh_prepare_dev(*t, C.R_FEATURE)
            ctx.normals_dev(*t, C.R, *nrm)
            ctx.fpfh_prepare_queries_dev(*t, *qs, C.R_FEATURE)
            ctx.fpfh_dev(*t, *nrm[:3], *qs, C.R_FEATURE, out)
            torch.cuda.synchronize(dev)
            seen.append(_stat(ctx, "fpfh_speculative_reruns") - before)
            on = O.normals(*xyz, C.R)
            _same_normals(nrm, on, f"scan {i}: normals")
            want = O.fpfh(*xyz, *on[:3], *q, C.R_FEATURE)
            bad = _rows_differ(out.cpu().numpy(), want)
            assert len(bad) == 0, f"scan {i}: rows {bad[:8].tolist()} differ from the oracle"
            with Context(0) as fresh:
                assert bits_equal(fresh.fpfh(*xyz, *on[:3], *q, C.R_FEATURE), want), i
    print("fpfh call order, reruns per scan", seen)
    # scan 3, compact on the stray scan's coarse hint: every point inside it, and the stray scan's exact
    # rebuild found its fat cell (3,000 points in one), so the radix builder is taken: no rerun
    lo, hi = C.bounds(s)
    assert C.cell_and_block_counts(s, C.R_FEATURE)[0].max() > C.FAT_CAP
    hlo, hhi = C.hint_bounds(lo, hi, C.R_FEATURE)
    assert (hlo < C.bounds(c)[0]).all() and (hhi > C.bounds(c)[1]).all()
    assert seen == [0, 0, 1, 0, 0]
