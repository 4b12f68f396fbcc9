"""3D shape contexts, unique shape contexts and SHOT's frames alone (pfx_shape_context / pfx_usc /
pfx_shot_lrf and their _dev forms, pfx_shape_context.hip) against the CPU restatement
(tests/cpp/shape_context_ref.cpp, pinned by tests/test_shape_context_ref.py): raw bits of every row of
desc and rf, and every statistic.  Shapes are the smallest that reach every path of the kernels:
wave-edge and chunk-edge neighbourhood sizes, the switch between the two passes at its exact capacity,
the capacity itself, bins that collide heavily, densities that reach beyond every query ball."""
import os

import numpy as np
import pytest

import list_edge_clouds as E
import pfh_cases as C
import shape_context_cases as K
import shape_context_ref as P
from parity import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = os.path.join(ROOT, "tests", "golden", "clouds")
STATS = ("neighbors", "kmax", "draws", "skipped_close", "support", "queued")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("shape_context_ref"))


def rows_of(a, rows):
    return tuple(v[rows] for v in a)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(got)} differ"


def all_nan(rows):
    return (bits(rows) == K.NAN_BITS).all()


def stats(ctx):
    return tuple(ctx.stat("sc_" + s) for s in STATS)


def check_sc(ctx, ref, xyz, nrm, q, r=K.R, rnd=None):
    """ctx.shape_context == the restatement: rows, frames and statistics; returns the restatement's."""
    want = P.shape_context(ref, *xyz, *nrm, *q, r, rnd=rnd)
    desc, rf = ctx.shape_context(*xyz, *nrm, *q, r, rnd=rnd)
    got = stats(ctx)
    same(desc, want.desc, "shape_context desc")
    same(rf, want.rf, "shape_context rf")
    assert got == tuple(want[2:]), (got, want[2:])
    return want


def check_usc(ctx, ref, xyz, q, frames, r=K.R):
    want = P.usc(ref, *xyz, *q, frames, r)
    desc, rf = ctx.usc(*xyz, *q, frames, r)
    got = stats(ctx)
    same(desc, want.desc, "usc desc")
    same(rf, want.rf, "usc rf")
    assert got == tuple(want[2:]), (got, want[2:])
    return want


def test_capacity_constant(ctx):
    assert ctx.stat("sc_cap_small") == P.CAP_SMALL


# ---- 1. the reference cloud ----

@pytest.fixture(scope="module")
def indoor(ctx, ref):
    """Indoor source with normals at 0.05: 64 seeded cloud rows and three points off the cloud, the far
    one in the middle of the list (the later rows' draws shift by one)."""
    from pcl_feature_extraction_amd.pcd import read_pcd
    c = read_pcd(os.path.join(CLOUDS, "indoor_source.pcd"))
    xyz = (c.x, c.y, c.z)
    nrm = tuple(ctx.normals(*xyz, 0.05)[:3])
    fin = np.flatnonzero(np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.z))
    rows = np.sort(np.random.default_rng(31).choice(fin, 64, replace=False))
    a, b = rows[0], rows[1]
    far = np.float32([[9.0e3, 9.0e3, 9.0e3]])
    beside = np.float32([[c.x[a] + 0.003, c.y[a] - 0.002, c.z[a] + 0.001], [c.x[b] - 0.01, c.y[b] + 0.01, c.z[b]]])
    q = tuple(np.concatenate([v[rows[:32]], far[:, i], v[rows[32:]], beside[:, i]]).astype(np.float32)
              for i, v in enumerate(xyz))
    return dict(xyz=xyz, normals=nrm, q=q, far=32, sc=P.shape_context(ref, *xyz, *nrm, *q, K.R))


def test_shape_context_on_the_reference_cloud(ctx, indoor):
    want = indoor["sc"]
    desc, rf = ctx.shape_context(*indoor["xyz"], *indoor["normals"], *indoor["q"], K.R)
    got = stats(ctx)
    same(desc, want.desc, "desc")
    same(rf, want.rf, "rf")
    assert got == tuple(want[2:])
    far = indoor["far"]
    assert all_nan(want.desc[far]) and not want.rf[far].any() and want.draws == 66
    assert np.isfinite(np.delete(want.desc, far, axis=0)).all() and want.neighbors > 66 * 100
    assert want.support > want.kmax and (np.delete(want.desc, far, axis=0) > 0).sum(axis=1).min() > 8


def test_shot_lrf_and_usc_on_the_reference_cloud(ctx, ref, indoor):
    xyz, q = indoor["xyz"], indoor["q"]
    rf = ctx.shot_lrf(*xyz, *q, K.R)
    _, rf_shot = ctx.shot(*xyz, *indoor["normals"], *q, K.R)
    same(rf, rf_shot, "shot_lrf against shot's rf")
    far = indoor["far"]
    assert all_nan(rf[far]) and np.isfinite(np.delete(rf, far, axis=0)).all()
    want = check_usc(ctx, ref, xyz, q, rf)
    assert all_nan(want.desc[far]) and not want.rf[far].any()       # a NaN frame: NaN row, zero rf
    assert np.array_equal(np.delete(want.rf, far, axis=0), np.delete(rf, far, axis=0))
    assert want.draws == 0 and want.neighbors == indoor["sc"].neighbors


# ---- 2. neighbourhood sizes ----

def blob_inputs(xyz, seed):
    n = len(xyz[0])
    return C.unit_normals(n, seed)


def test_neighbourhood_sizes_at_wave_and_chunk_edges(ctx, ref):
    ks = (1, 2, 63, 64, 65, 255, 256, 257)
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), 810 + 2 * s) for s, k in enumerate(ks)]
    xyz, nrm, rows = C.concat(parts)
    qr = np.array([r for lo, hi in rows for r in sorted(set(E.three_rows(lo, hi)))])
    want = check_sc(ctx, ref, xyz, nrm, rows_of(xyz, qr), E.R)
    assert want.kmax == 257 and want.draws == len(qr) and np.isfinite(want.desc).all()
    assert not want.desc[0].any()          # k = 1: only itself, skipped
    frames = ctx.shot_lrf(*xyz, *rows_of(xyz, qr), E.R)
    check_usc(ctx, ref, xyz, rows_of(xyz, qr), frames, E.R)


def test_pass_boundary(ctx, ref):
    cap = ctx.stat("sc_cap_small")
    xyz, blobs = E.exact_k_blobs(caps=[cap], deltas=(-1, 0, 1))
    nrm = blob_inputs(xyz, 820)
    qr = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    assert [k for k, _, _ in blobs] == [cap - 1, cap, cap + 1]
    want = check_sc(ctx, ref, xyz, nrm, rows_of(xyz, qr), E.R)
    assert want.kmax == cap + 1 and want.queued == 3     # only the blob above the capacity
    frames = ctx.shot_lrf(*xyz, *rows_of(xyz, qr), E.R)
    _, rf_shot = ctx.shot(*xyz, *nrm, *rows_of(xyz, qr), E.R)
    same(frames, rf_shot, "shot_lrf against shot's rf")
    assert check_usc(ctx, ref, xyz, rows_of(xyz, qr), frames, E.R).queued == 3


def test_capacity(ctx, ref):
    """16,384 neighbours pass; 16,385 give PFX_ERR_CAPACITY, and the next call is unaffected."""
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(0, 1))
    (k0, lo0, hi0), (k1, lo1, hi1) = blobs
    assert (k0, k1) == (16384, 16385)
    nrm = blob_inputs(xyz, 830)
    q, bad = rows_of(xyz, [lo0, hi0 - 1]), rows_of(xyz, [lo0, lo1])
    want = check_sc(ctx, ref, xyz, nrm, q, E.R)
    assert want.kmax == 16384 and want.queued == 2
    with pytest.raises(PfxError) as e:
        ctx.shape_context(*xyz, *nrm, *bad, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value)
    same(ctx.shape_context(*xyz, *nrm, *q, E.R)[0], want.desc, "shape_context after the error")
    frames = ctx.shot_lrf(*xyz, *q, E.R)
    assert np.isfinite(frames).all()
    with pytest.raises(PfxError) as e:
        ctx.shot_lrf(*xyz, *bad, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value)
    same(ctx.shot_lrf(*xyz, *q, E.R), frames, "shot_lrf after the error")
    check_usc(ctx, ref, xyz, q, frames, E.R)
    with pytest.raises(PfxError) as e:
        ctx.usc(*xyz, *bad, frames, E.R)
    assert e.value.code == PFX_ERR_CAPACITY


# ---- 3. the order ----

def test_order(ctx, ref):
    """Dense blobs of 1,100 points: the restatement walked backwards differs in some bin, so equal
    bits show that every bin was summed in neighbour order."""
    c = K.order_case()
    want = check_sc(ctx, ref, c["xyz"], c["normals"], c["q"])
    back = P.shape_context(ref, *c["xyz"], *c["normals"], *c["q"], K.R, reversed_order=True)
    assert want.kmax == c["k"] >= 1024 and (bits(want.desc) != bits(back.desc)).any()
    frames = ctx.shot_lrf(*c["xyz"], *c["q"], K.R)
    uw = check_usc(ctx, ref, c["xyz"], c["q"], frames)
    ub = P.usc(ref, *c["xyz"], *c["q"], frames, K.R, reversed_order=True)
    assert (bits(uw.desc) != bits(ub.desc)).any()


# ---- 4. the density ----

def test_density_reaches_beyond_every_query_ball(ctx, ref):
    c = K.rim_case()
    want = check_sc(ctx, ref, c["xyz"], c["normals"], c["q"], rnd=np.float32([1, 0, 0.5]))
    (b,) = np.flatnonzero(want.desc[0])
    t = P.tables(ref, K.R, K.RMIN)
    assert want.desc[0, b] == (np.float32(1) / np.float32(c["density"])) * t.lut[(b % 165) // 15, b % 15]
    assert want.support == 2     # the NaN point beside the neighbour is counted nowhere


def test_density_on_a_cloud_with_nan_points(ctx, ref):
    c = K.order_case(k=300, blobs=2, seed=740)
    x = c["xyz"][0].copy()
    x[5::7] = np.nan
    xyz = (x, c["xyz"][1], c["xyz"][2])
    want = check_sc(ctx, ref, xyz, c["normals"], c["q"])
    assert want.kmax < 300 and np.isfinite(want.desc).all()


# ---- 5. the contract cases ----

def test_contract_cases(ctx, ref):
    one = np.float32([1.0, 0.0, 0.5])
    q0 = K.points(K.Q0)
    for normal, rnd in (((0, 0, 1), (3, 4, 9)), ((0, 1, 0), (3, 9, 4)), ((1, 0, 0), (9, 3, 4)), ((0, 0, 0), (3, 0, 4)),
                        ((np.nan, 0, 1), (1, 0, 0.5))):
        xyz, nrm = K.lone_neighbour(normal=normal)
        want = check_sc(ctx, ref, xyz, nrm, q0, rnd=np.float32(rnd))
        assert np.isfinite(want.desc).all() and len(np.flatnonzero(want.desc[0])) == 1
    for dz in (2 * K.STEP, -2 * K.STEP):                                  # on the normal's axis: theta 0 and 180
        xyz, nrm = K.lone_neighbour(step=(0.0, 0.0, dz))
        check_sc(ctx, ref, xyz, nrm, q0, rnd=one)
    e = 2.0 ** -12                                                         # the skip on either side of epsilon
    want = check_sc(ctx, ref, K.points(K.Q0, K.offset(e), K.offset(0.0, e, e)), K.vectors(3, (0, 0, 1)), q0, rnd=one)
    assert want.skipped_close == 2
    p = K.offset(K.STEP, K.STEP, K.STEP)                                   # duplicates
    want = check_sc(ctx, ref, K.points(K.Q0, K.Q0, p, p, p), K.vectors(5, (0, 0, 1)), q0, rnd=one)
    assert want.skipped_close == 2 and np.flatnonzero(want.desc[0]).tolist() == [217]


def test_special_rows(ctx, ref):
    xyz, nrm = K.lone_neighbour()
    q = K.points((9.0e3, 9.0e3, 9.0e3), (np.nan, 2.0, 3.0), K.Q0)
    want = check_sc(ctx, ref, xyz, nrm, q, rnd=np.float32([1, 0, 0.5] + [7] * 6))
    assert all_nan(want.desc[:2]) and not want.rf[:2].any() and want.draws == 1
    frames = np.float32([[1, 0, 0, 0, 1, 0, 0, 0, 1]] * 3)
    want = check_usc(ctx, ref, xyz, q, frames)
    assert not want.desc[0].any() and all_nan(want.desc[1])
    for bad in (0, 3, 6):
        fr = frames.copy()
        fr[2, bad] = np.nan
        assert all_nan(check_usc(ctx, ref, xyz, q, fr).desc[2])
    # no query, no surface
    d, f = ctx.shape_context(*xyz, *nrm, *rows_of(xyz, slice(0, 0)), K.R)
    assert d.shape == (0, 1980) and f.shape == (0, 9)
    none = rows_of(xyz, slice(0, 0))
    d, f = ctx.shape_context(*none, *none, *q, K.R)
    assert all_nan(d) and not f.any() and ctx.stat("sc_neighbors") == 0
    d, f = ctx.usc(*none, *q, frames, K.R)
    assert not d[[0, 2]].any() and all_nan(d[1]) and np.array_equal(f[[0, 2]], frames[[0, 2]]) and not f[1].any()
    assert all_nan(ctx.shot_lrf(*none, *q, K.R))


# ---- 6. the random stream ----

def test_rnd_stream(ctx, indoor):
    from pcl_feature_extraction_amd import uniform01_stream
    xyz, nrm, q = indoor["xyz"], indoor["normals"], indoor["q"]
    nq = len(q[0])
    desc, rf = ctx.shape_context(*xyz, *nrm, *q, K.R, rnd=uniform01_stream(12345, 3 * nq))
    same(desc, indoor["sc"].desc, "the stated stream against the default one")
    same(rf, indoor["sc"].rf, "rf")
    _, rf2 = ctx.shape_context(*xyz, *nrm, *q, K.R, rnd=uniform01_stream(54321, 3 * nq))
    live = np.flatnonzero(np.isfinite(rf).all(axis=1) & rf.any(axis=1))
    assert len(live) >= 60 and (bits(rf2[live, :3]) != bits(rf[live, :3])).any(axis=1).all()
    assert np.array_equal(bits(rf2[:, 6:]), bits(rf[:, 6:]))     # the normal does not come from the stream


# ---- 7. the _dev forms ----

def test_dev_forms_on_a_callers_stream(ref, indoor):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    s, sn, q = up(*indoor["xyz"]), up(*indoor["normals"]), up(*indoor["q"])
    nq = len(indoor["q"][0])
    new = lambda w: torch.full((nq, w), -1.0, dtype=torch.float32, device=dev)  # noqa: E731
    d, f, ud, uf, lrf = [new(1980), new(1980)], [new(9), new(9)], new(1980), new(9), new(9)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    want = indoor["sc"]
    with Context(0) as c:
        c.set_stream(stream.cuda_stream)
        for i in range(2):
            c.shape_context_dev(*s, *sn, *q, K.R, d[i], f[i])
        c.synchronize()
        assert tuple(c.stat("sc_" + n) for n in STATS) == tuple(want[2:])
        c.shot_lrf_dev(*s, *q, K.R, lrf)
        c.usc_dev(*s, *q, lrf, K.R, ud, uf)    # the frames never leave the device
        c.synchronize()
        assert c.stat("sc_draws") == 0 and c.stat("sc_neighbors") == want.neighbors
    for i in range(2):
        same(d[i].cpu().numpy(), want.desc, "shape_context_dev")
        same(f[i].cpu().numpy(), want.rf, "shape_context_dev rf")
    frames = lrf.cpu().numpy()
    uw = P.usc(ref, *indoor["xyz"], *indoor["q"], frames, K.R)
    same(ud.cpu().numpy(), uw.desc, "usc_dev")
    same(uf.cpu().numpy(), uw.rf, "usc_dev rf")


def test_dev_forms_report_a_late_capacity_error_at_synchronize(ref):
    import torch
    from pcl_feature_extraction_amd import Context, PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(1,))
    (k, lo, hi), = blobs
    nrm = blob_inputs(xyz, 870)
    rows = [0, lo]       # the anchor (a lone point) and a point of the blob beyond capacity
    s, sn, q = up(*xyz), up(*nrm), up(*rows_of(xyz, rows))
    d = torch.zeros((2, 1980), dtype=torch.float32, device=dev)
    f = torch.zeros((2, 9), dtype=torch.float32, device=dev)
    fr = torch.zeros((2, 9), dtype=torch.float32, device=dev)
    fr[:, 0] = fr[:, 4] = fr[:, 8] = 1.0
    torch.cuda.synchronize()
    with Context(0) as c:
        for launch in (lambda: c.shape_context_dev(*s, *sn, *q, E.R, d, f),
                       lambda: c.usc_dev(*s, *q, fr, E.R, d, f),
                       lambda: c.shot_lrf_dev(*s, *q, E.R, f)):
            launch()     # returns without the error
            with pytest.raises(PfxError) as e:
                c.synchronize()
            assert e.value.code == PFX_ERR_CAPACITY and str(k) in str(e.value)
            c.synchronize()   # reported once
        ok = up(*rows_of(xyz, [0]))
        c.shape_context_dev(*s, *sn, *ok, E.R, d[:1], f[:1])
        c.synchronize()
        want = P.shape_context(ref, *xyz, *nrm, *rows_of(xyz, [0]), E.R)
        assert c.stat("sc_kmax") == want.kmax == 1
    same(d[:1].cpu().numpy(), want.desc, "shape_context_dev after the error")
    same(f[:1].cpu().numpy(), want.rf, "rf after the error")


# ---- 8. invalid arguments ----

def test_invalid_arguments(ctx):
    import ctypes
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID
    xyz, nrm = K.lone_neighbour()
    frames = np.float32([[1, 0, 0, 0, 1, 0, 0, 0, 1]] * 2)
    ctx.shape_context(*xyz, *nrm, *xyz, K.R)
    before = stats(ctx)
    for kw in (dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(min_radius=0.0), dict(point_density_radius=0.0),
               dict(min_radius=0.09), dict(point_density_radius=float("nan"))):
        r = kw.pop("r", K.R)
        with pytest.raises(PfxError) as e:
            ctx.shape_context(*xyz, *nrm, *xyz, r, **kw)
        assert e.value.code == PFX_ERR_INVALID, kw
        with pytest.raises(PfxError) as e:
            ctx.usc(*xyz, *xyz, frames, r, **kw)
        assert e.value.code == PFX_ERR_INVALID, kw
    with pytest.raises(PfxError) as e:
        ctx.shot_lrf(*xyz, *xyz, 0.0)
    assert e.value.code == PFX_ERR_INVALID
    lib, p = ctx._lib, lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    d, f = np.empty((2, 1980), np.float32), np.empty((2, 9), np.float32)
    a = [p(v) for v in (*xyz, *nrm)] + [2] + [p(v) for v in xyz] + [2, K.R, K.RMIN, K.RHO, None, p(d), p(f)]
    assert lib.pfx_shape_context(ctx.h, *a) == 0          # a null rnd is the default stream
    for null in (0, 3, 7, 15, 16):
        b = list(a)
        b[null] = None
        assert lib.pfx_shape_context(ctx.h, *b) == PFX_ERR_INVALID
    b = list(a)
    b[6] = -1
    assert lib.pfx_shape_context(ctx.h, *b) == PFX_ERR_INVALID
    a = [p(v) for v in xyz] + [2] + [p(v) for v in xyz] + [p(frames), 2, K.R, K.RMIN, K.RHO, p(d), p(f)]
    for null in (0, 4, 7, 12, 13):
        b = list(a)
        b[null] = None
        assert lib.pfx_usc(ctx.h, *b) == PFX_ERR_INVALID
    a = [p(v) for v in xyz] + [2] + [p(v) for v in xyz] + [2, K.R, p(f)]
    for null in (0, 4, 9):
        b = list(a)
        b[null] = None
        assert lib.pfx_shot_lrf(ctx.h, *b) == PFX_ERR_INVALID
    assert lib.pfx_rng_uniform01(1, -1, 1, p(f)) == PFX_ERR_INVALID
    assert lib.pfx_rng_uniform01(1, 0, 1, None) == PFX_ERR_INVALID
    assert stats(ctx) == before      # nothing was launched
