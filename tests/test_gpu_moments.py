"""Moment invariants and principal curvatures (pfx_moment_invariants / pfx_principal_curvatures and
their _dev forms, pfx_moments.hip) against the CPU restatements (tests/cpp/moments_ref.cpp, pinned by
tests/test_moments_ref.py): raw bits of every row of both outputs and every statistic.  Shapes are
the smallest that reach every path of the kernel: wave-edge and chunk-edge neighbourhood sizes, the
switch between the two passes at its exact capacity, the second pass's stride loop, the capacity
itself."""
import os

import numpy as np
import pytest

import list_edge_clouds as E
import moments_cases as K
import moments_ref as P
import pfh_cases as C
from parity import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = os.path.join(ROOT, "tests", "golden", "clouds")
FAR = (9.0e3, 9.0e3, 9.0e3)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("moments_ref"))


def rows_of(a, rows):
    return tuple(v[rows] for v in a)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(got)} differ"


def all_nan(rows):
    return (bits(rows) == K.NAN_BITS).all()


def stats(ctx, what):
    return tuple(ctx.stat(what + s) for s in ("_neighbors", "_kmax", "_queued"))


def queued(ctx, want):
    """The rows above the first pass's capacity."""
    return int((want.k > ctx.stat("moments_cap_small")).sum())


def check_moments(ctx, ref, xyz, q, r=K.R, queued_rows=0):
    """ctx.moment_invariants == the restatement, rows and statistics; returns the restatement's result."""
    want = P.moments(ref, *xyz, *q, r)
    same(ctx.moment_invariants(*xyz, *q, r), want.out, "moment invariants")
    assert queued(ctx, want) == queued_rows
    assert stats(ctx, "moments") == (want.neighbors, want.kmax, queued_rows)
    return want


def check_curvatures(ctx, ref, xyz, nrm, q, qn, r=K.R, queued_rows=0):
    want = P.curvatures(ref, *xyz, *nrm, *q, *qn, r)
    same(ctx.principal_curvatures(*xyz, *nrm, *q, *qn, r), want.out, "principal curvatures")
    assert queued(ctx, want) == queued_rows
    assert stats(ctx, "pcurv") == (want.neighbors, want.kmax, queued_rows)
    return want


# ---- 1. the reference cloud ----

@pytest.fixture(scope="module")
def indoor(ctx, ref):
    """Indoor source at its ISS keypoints and one far point, r = 0.08, normals at 0.05 (the
    restatement's rows, once)."""
    from pcl_feature_extraction_amd.pcd import read_pcd
    c = read_pcd(os.path.join(CLOUDS, "indoor_source.pcd"))
    xyz = (c.x, c.y, c.z)
    nrm = tuple(ctx.normals(*xyz, 0.05)[:3])
    res = ctx.cloud_resolution(*xyz)
    kp = np.asarray(ctx.iss_keypoints(*xyz, 6 * res, 4 * res), np.int64)
    assert len(kp) > 500
    q = tuple(np.append(v[kp], np.float32(f)) for v, f in zip(xyz, FAR))
    qn = tuple(np.append(v[kp], v[kp[0]]) for v in nrm)
    return dict(xyz=xyz, normals=nrm, q=q, qn=qn, mi=P.moments(ref, *xyz, *q, 0.08),
                pc=P.curvatures(ref, *xyz, *nrm, *q, *qn, 0.08))


def test_reference_cloud_at_its_keypoints(ctx, indoor):
    xyz, nrm, q, qn = indoor["xyz"], indoor["normals"], indoor["q"], indoor["qn"]
    want = indoor["mi"]
    same(ctx.moment_invariants(*xyz, *q, 0.08), want.out, "moment invariants")
    assert stats(ctx, "moments") == (want.neighbors, want.kmax, queued(ctx, want))
    assert all_nan(want.out[-1]) and np.isfinite(want.out[:-1]).all() and want.neighbors > 100 * len(want.out)
    want = indoor["pc"]
    same(ctx.principal_curvatures(*xyz, *nrm, *q, *qn, 0.08), want.out, "principal curvatures")
    assert stats(ctx, "pcurv") == (want.neighbors, want.kmax, queued(ctx, want))
    assert all_nan(want.out[-1]) and np.isfinite(want.out[:-1]).all(axis=1).sum() > 0.9 * len(want.out)
    assert want.detours >= 1   # (root2 * scale) / scale differs from root2 on some rows of this very cloud


# ---- 2. neighbourhood sizes ----

def test_neighbourhood_sizes_at_wave_and_chunk_edges(ctx, ref):
    ks = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513)
    c = K.blobs_case(ks, 630)
    xyz, nrm = c["xyz"], c["normals"]
    qr = np.array([r for lo, hi in c["rows"] for r in sorted(set(E.three_rows(lo, hi)))])
    q, qn = rows_of(xyz, qr), C.unit_normals(len(qr), 629)
    want = check_moments(ctx, ref, xyz, q)
    assert want.kmax == 513 and np.isfinite(want.out).all() and not want.out[0].any()
    want = check_curvatures(ctx, ref, xyz, nrm, q, qn)
    assert want.kmax == 513 and all_nan(want.out[0, :3]) and np.isfinite(want.out[1:]).all()


def test_pass_boundary(ctx, ref):
    cap = ctx.stat("moments_cap_small")
    assert cap == 2048
    xyz, blobs = E.exact_k_blobs(caps=[cap], deltas=(-1, 0, 1))
    n = len(xyz[0])
    nrm = C.unit_normals(n, 642)
    qr = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    assert [k for k, _, _ in blobs] == [cap - 1, cap, cap + 1]
    q, qn = rows_of(xyz, qr), C.unit_normals(len(qr), 643)
    want = check_moments(ctx, ref, xyz, q, E.R, queued_rows=3)     # only the blob above the capacity
    assert want.kmax == cap + 1 and np.isfinite(want.out).all()
    want = check_curvatures(ctx, ref, xyz, nrm, q, qn, E.R, queued_rows=3)
    assert want.kmax == cap + 1 and np.isfinite(want.out).all()


def test_second_pass_stride_loop(ctx, ref):
    """One blob of 2,049 points, every point a query: 2,049 queued queries over the second pass's 256
    workgroups."""
    xyz, blobs = E.exact_k_blobs(caps=[2048], deltas=(1,))
    (k, lo, hi), = blobs
    n = len(xyz[0])
    nrm = C.unit_normals(n, 652)
    q, qn = rows_of(xyz, slice(lo, hi)), rows_of(nrm, slice(lo, hi))
    assert k == 2049 and len(q[0]) == 2049
    want = check_moments(ctx, ref, xyz, q, E.R, queued_rows=2049)
    assert want.neighbors == 2049 * 2049
    check_curvatures(ctx, ref, xyz, nrm, q, qn, E.R, queued_rows=2049)


def test_capacity(ctx, ref):
    """16,384 neighbours pass; 16,385 give PFX_ERR_CAPACITY, and the next call is unaffected."""
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(0, 1))
    (k0, lo0, hi0), (k1, lo1, hi1) = blobs
    assert (k0, k1) == (16384, 16385)
    nrm = C.unit_normals(len(xyz[0]), 662)
    q, qn = rows_of(xyz, [lo0, hi0 - 1]), rows_of(nrm, [lo0, hi0 - 1])
    bad = rows_of(xyz, [lo0, lo1])
    mw = check_moments(ctx, ref, xyz, q, E.R, queued_rows=2)
    assert mw.kmax == 16384
    with pytest.raises(PfxError) as e:
        ctx.moment_invariants(*xyz, *bad, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value) and "16384" in str(e.value)
    same(ctx.moment_invariants(*xyz, *q, E.R), mw.out, "moment invariants after the error")
    pw = check_curvatures(ctx, ref, xyz, nrm, q, qn, E.R, queued_rows=2)
    assert pw.kmax == 16384
    with pytest.raises(PfxError) as e:
        ctx.principal_curvatures(*xyz, *nrm, *bad, *qn, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value) and "16384" in str(e.value)
    same(ctx.principal_curvatures(*xyz, *nrm, *q, *qn, E.R), pw.out, "principal curvatures after the error")


def test_order(ctx, ref):
    """A few hundred neighbours a row: the bits equal the restatement's and differ from those of its
    reversed walk."""
    c = K.order_case()
    want = check_moments(ctx, ref, c["xyz"], c["q"])
    rev = P.moments(ref, *c["xyz"], *c["q"], K.R, reversed_order=True)
    assert (bits(want.out) != bits(rev.out)).any()
    want = check_curvatures(ctx, ref, c["xyz"], c["normals"], c["q"], c["qnormals"])
    rev = P.curvatures(ref, *c["xyz"], *c["normals"], *c["q"], *c["qnormals"], K.R, reversed_order=True)
    assert (bits(want.out) != bits(rev.out)).any()


def test_the_eigenvalue_detour(ctx, ref):
    c = K.smooth_blobs()
    want = check_curvatures(ctx, ref, c["xyz"], c["normals"], c["xyz"], c["normals"])
    assert want.detours >= 1


# ---- 3. the special rows ----

def test_contract_rows(ctx, ref):
    q0 = K.points(K.Q0)
    for abc in ((2.0 ** -6, 2.0 ** -7, 2.0 ** -5), (2.0 ** -5, 2.0 ** -8, 2.0 ** -7)):
        xyz, row = K.axis_case(*abc)
        assert np.array_equal(check_moments(ctx, ref, xyz, q0).out[0], np.float32(row))
    xyz, row = K.diagonal_case()
    assert np.array_equal(check_moments(ctx, ref, xyz, q0).out[0], np.float32(row))
    for m in (1, 4):
        xyz, nrm, row = K.spread_case(m)
        assert np.array_equal(check_curvatures(ctx, ref, xyz, nrm, q0, K.vectors(1, K.Z)).out[0], np.float32(row))


def test_special_rows(ctx, ref):
    xyz, nrm, _ = K.spread_case(2)
    # a far query, a NaN query coordinate, the centre with a NaN query normal
    q = K.points(K.Q0, FAR, (np.nan, 2.0, 3.0), K.Q0)
    qn = K.f32([0.0, 0.0, 0.0, np.nan], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0])
    want = check_moments(ctx, ref, xyz, q)
    assert all_nan(want.out[1:3]) and np.isfinite(want.out[[0, 3]]).all()
    want = check_curvatures(ctx, ref, xyz, nrm, q, qn)
    assert all_nan(want.out[1:]) and np.isfinite(want.out[0]).all()
    # a NaN normal among the neighbours
    n = tuple(v.copy() for v in nrm)
    n[1][3] = np.nan
    assert all_nan(check_curvatures(ctx, ref, xyz, n, K.points(K.Q0), K.vectors(1, K.Z)).out)
    # duplicate points, k = 1, equal normals
    dup = K.points(K.Q0, K.Q0, K.offset(K.STEP), K.offset(K.STEP), K.offset(0.0, -K.STEP))
    check_moments(ctx, ref, dup, dup)
    check_curvatures(ctx, ref, dup, C.unit_normals(5, 670), dup, C.unit_normals(5, 671))
    one = K.points(K.Q0)
    assert not check_moments(ctx, ref, one, one).out.any()
    for xyz, k in ((one, 1), (K.ring(8), 8)):
        want = check_curvatures(ctx, ref, xyz, K.vectors(k, (0.5, 0.25, 1.0)), one, K.vectors(1, K.Z))
        assert all_nan(want.out[0, :3]) and not want.out[0, 3:].any() and not np.signbit(want.out[0, 3:]).any()
    # a non-finite surface point is no neighbour; no surface at all; no query at all
    xyz, _ = K.axis_case()
    x = np.append(xyz[0], np.float32(np.nan))
    s = (x, np.append(xyz[1], np.float32(2.0)), np.append(xyz[2], np.float32(3.0)))
    assert check_moments(ctx, ref, s, s).kmax == 7
    check_curvatures(ctx, ref, s, C.unit_normals(8, 672), s, C.unit_normals(8, 673))
    none = rows_of(one, slice(0, 0))
    assert all_nan(ctx.moment_invariants(*none, *one, K.R)) and stats(ctx, "moments") == (0, 0, 0)
    assert all_nan(ctx.principal_curvatures(*none, *none, *one, *K.vectors(1, K.Z), K.R))
    assert stats(ctx, "pcurv") == (0, 0, 0)
    assert ctx.moment_invariants(*one, *none, K.R).shape == (0, 3)
    assert ctx.principal_curvatures(*one, *K.vectors(1, K.Z), *none, *none, K.R).shape == (0, 5)


# ---- 4. the _dev forms ----

def test_dev_forms_on_a_callers_stream(indoor):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    s, sn, q, qn = up(*indoor["xyz"]), up(*indoor["normals"]), up(*indoor["q"]), up(*indoor["qn"])
    nq = len(indoor["q"][0])
    mi = [torch.full((nq, 3), -1.0, dtype=torch.float32, device=dev) for _ in range(2)]
    pc = [torch.full((nq, 5), -1.0, dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.set_stream(stream.cuda_stream)
        # no host wait between these launches and synchronize()
        c.moment_invariants_dev(*s, *q, 0.08, mi[0])
        c.principal_curvatures_dev(*s, *sn, *q, *qn, 0.08, pc[0])
        c.moment_invariants_dev(*s, *q, 0.08, mi[1])
        c.principal_curvatures_dev(*s, *sn, *q, *qn, 0.08, pc[1])
        c.synchronize()
        for what, want in (("moments", indoor["mi"]), ("pcurv", indoor["pc"])):
            assert (c.stat(what + "_neighbors"), c.stat(what + "_kmax")) == (want.neighbors, want.kmax)
    for o in mi:
        same(o.cpu().numpy(), indoor["mi"].out, "moment_invariants_dev")
    for o in pc:
        same(o.cpu().numpy(), indoor["pc"].out, "principal_curvatures_dev")


def test_dev_forms_report_a_late_capacity_error_at_synchronize(ref):
    import torch
    from pcl_feature_extraction_amd import Context, PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(1,))
    (k, lo, hi), = blobs
    nrm = C.unit_normals(len(xyz[0]), 682)
    rows = [0, lo]       # the anchor (a lone point) and a point of the blob beyond capacity
    s, sn = up(*xyz), up(*nrm)
    q, qn = up(*rows_of(xyz, rows)), up(*rows_of(nrm, rows))
    out_m = torch.zeros((2, 3), dtype=torch.float32, device=dev)
    out_p = torch.zeros((2, 5), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        for launch in (lambda: c.moment_invariants_dev(*s, *q, E.R, out_m),
                       lambda: c.principal_curvatures_dev(*s, *sn, *q, *qn, E.R, out_p)):
            launch()     # returns without the error
            with pytest.raises(PfxError) as e:
                c.synchronize()
            assert e.value.code == PFX_ERR_CAPACITY and str(k) in str(e.value)
            c.synchronize()   # reported once
        # the next call is unaffected
        ok, okn = up(*rows_of(xyz, [0])), up(*rows_of(nrm, [0]))
        c.principal_curvatures_dev(*s, *sn, *ok, *okn, E.R, out_p[:1])
        c.synchronize()
        want = P.curvatures(ref, *xyz, *nrm, *rows_of(xyz, [0]), *rows_of(nrm, [0]), E.R)
        assert c.stat("pcurv_kmax") == want.kmax == 1
    same(out_p[:1].cpu().numpy(), want.out, "principal_curvatures_dev after the error")


# ---- 5. invalid arguments ----

def test_invalid_arguments(ctx):
    import ctypes
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID, PFX_OK
    c = K.order_case(k=8, blobs=1)
    xyz, nrm = c["xyz"], c["normals"]
    ctx.moment_invariants(*xyz, *xyz, K.R)
    ctx.principal_curvatures(*xyz, *nrm, *xyz, *nrm, K.R)
    before = ctx.stat("moments_kmax"), ctx.stat("pcurv_kmax")
    assert before == (8, 8)
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(PfxError) as e:
            ctx.moment_invariants(*xyz, *xyz, r)
        assert e.value.code == PFX_ERR_INVALID
        with pytest.raises(PfxError) as e:
            ctx.principal_curvatures(*xyz, *nrm, *xyz, *nrm, r)
        assert e.value.code == PFX_ERR_INVALID
    # null pointers and negative sizes, straight at the C-ABI
    lib, p = ctx._lib, lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = np.empty((8, 5), np.float32)
    a = [p(v) for v in xyz] + [8] + [p(v) for v in xyz] + [8, K.R, p(out)]
    for null in (0, 2, 4, 6, 9):
        b = list(a)
        b[null] = None
        assert lib.pfx_moment_invariants(ctx.h, *b) == PFX_ERR_INVALID
    for size in (3, 7):
        b = list(a)
        b[size] = -1
        assert lib.pfx_moment_invariants(ctx.h, *b) == PFX_ERR_INVALID
    a = [p(v) for v in (*xyz, *nrm)] + [8] + [p(v) for v in (*xyz, *nrm)] + [8, K.R, p(out)]
    for null in (0, 3, 5, 7, 10, 12, 15):
        b = list(a)
        b[null] = None
        assert lib.pfx_principal_curvatures(ctx.h, *b) == PFX_ERR_INVALID
    for size in (6, 13):
        b = list(a)
        b[size] = -1
        assert lib.pfx_principal_curvatures(ctx.h, *b) == PFX_ERR_INVALID
    # nq = 0 succeeds without a launch, null query pointers and all
    b = list(a)
    b[7:14] = [None] * 6 + [0]
    b[15] = None
    assert lib.pfx_principal_curvatures(ctx.h, *b) == PFX_OK
    # nothing was launched: the statistics are those of the last valid calls, and the context works
    assert (ctx.stat("moments_kmax"), ctx.stat("pcurv_kmax")) == before
    assert np.isfinite(ctx.moment_invariants(*xyz, *xyz, K.R)).all()
