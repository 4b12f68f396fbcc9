"""BOARD local reference frames (pfx_board_lrf and its _dev form, pfx_board.hip) against the CPU
restatement (tests/cpp/board_ref.cpp, pinned by tests/test_board_ref.py): raw bits of every row and
every statistic.  Shapes are the smallest that reach every path of the kernel: the k < 6 rule,
wave-edge and chunk-edge neighbourhood sizes, ties of the minimum across waves and chunks, the
switch between the two passes at its exact capacity, the second pass's stride loop, the capacity
itself, the three kinds of tangent radius."""
import os

import numpy as np
import pytest

import board_cases as K
import board_ref as P
import list_edge_clouds as E
import match_model as M
import pfh_cases as C
import shape_context_ref as SC
from parity import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = os.path.join(ROOT, "tests", "golden", "clouds")
FAR = (9.0e3, 9.0e3, 9.0e3)
CASES = K.closed_form_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("board_ref"))


def rows_of(a, rows):
    return tuple(v[rows] for v in a)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(got)} differ"


def all_nan(rows):
    return (bits(rows) == K.NAN_BITS).all()


def stats(ctx):
    return tuple(ctx.stat("board" + s) for s in ("_neighbors", "_kmax", "_queued"))


def check(ctx, ref, xyz, nrm, q, r, tangent_radius=0.0, margin_thresh=0.85, queued_rows=0):
    """ctx.board_lrf == the restatement, rows and statistics; returns the restatement's result."""
    want = P.frames(ref, *xyz, *nrm, *q, r, tangent_radius, margin_thresh)
    same(ctx.board_lrf(*xyz, *nrm, *q, r, tangent_radius, margin_thresh), want.rf, "board frames")
    assert int((want.k > ctx.stat("board_cap_small")).sum()) == queued_rows
    assert stats(ctx) == (want.neighbors, want.kmax, queued_rows)
    return want


# ---- 1. the closed forms ----

@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_closed_form_rows(ctx, ref, case):
    _, xyz, nrm, tangent_radius, row = case
    want = check(ctx, ref, xyz, nrm, K.points(K.Q0), K.R, tangent_radius)
    assert np.array_equal(K.got_bits(want.rf[0]), K.row_bits(row))


def test_margin_rules(ctx, ref):
    """A margin neighbour with a NaN normal blocks the fallback; margin_thresh 0 and 1."""
    q = K.points(K.Q0)
    xyz, nrm = K.patch(K.BASE + ((14, 0), (-14, 0)), special={7: K.NAN3, 8: K.NAN3, K.TILTED_ROW: K.TILT})
    assert all_nan(check(ctx, ref, xyz, nrm, q, K.R, K.R).rf)
    xyz, nrm = K.patch(K.BASE)
    assert check(ctx, ref, xyz, nrm, q, K.R, K.R, margin_thresh=0.0).chosen[0] == 1
    want = check(ctx, ref, xyz, nrm, q, K.R, K.R, margin_thresh=1.0)
    assert want.chosen[0] == 0 and all_nan(want.rf[0, :6]) and np.isfinite(want.rf[0, 6:]).all()


def test_special_queries(ctx, ref):
    xyz, nrm = K.patch(K.BASE)
    q = K.points(K.Q0, FAR, (np.nan, 2.0, 3.0), (1.0, np.inf, 3.0))
    want = check(ctx, ref, xyz, nrm, q, K.R)
    assert np.isfinite(want.rf[0]).all() and all_nan(want.rf[1:])
    # a non-finite surface point is nobody's neighbour
    x = np.append(xyz[0], np.float32(np.nan))
    s = (x, np.append(xyz[1], np.float32(2.0)), np.append(xyz[2], np.float32(3.0)))
    n = tuple(np.append(v, np.float32(1.0)) for v in nrm)
    assert check(ctx, ref, s, n, s, K.R).kmax == 7
    # the gathered count is that of the larger radius, whichever it is
    xyz, nrm = K.patch(K.BASE + ((14, 0), (-14, 0)))
    assert check(ctx, ref, xyz, nrm, K.points(K.Q0), K.TR, K.R).kmax == 9
    assert check(ctx, ref, xyz, nrm, K.points(K.Q0), K.R, K.TR).kmax == 9
    assert check(ctx, ref, xyz, nrm, K.points(K.Q0), K.TR).kmax == 6


# ---- 2. neighbourhood sizes ----

def test_neighbourhood_sizes_at_the_rule_and_at_wave_and_chunk_edges(ctx, ref):
    ks = (5, 6, 63, 64, 65, 255, 256, 257, 513)
    c = K.blobs_case(ks, 720)
    xyz, nrm = c["xyz"], c["normals"]
    qr = np.array([r for lo, hi in c["rows"] for r in sorted(set(E.three_rows(lo, hi)))])
    want = check(ctx, ref, xyz, nrm, rows_of(xyz, qr), C.R)
    assert want.kmax == 513 and sorted(set(want.k.tolist())) == sorted(ks)
    assert all_nan(want.rf[want.k == 5]) and np.isfinite(want.rf[want.k >= 6]).all()


def test_ties_of_the_minimum_go_to_the_first(ctx, ref):
    xyz, nrm, q, nb, first = K.tie_case()
    want = check(ctx, ref, xyz, nrm, q, C.R)
    assert want.chosen[0] == nb[first] and first == 100 and len(nb) == 320
    # every normal equal: the nearest neighbour with d2 > 0 wins over 318 others
    one = K.f32(*(np.full(320, v) for v in (0.36, 0.48, 0.8)))
    assert check(ctx, ref, xyz, one, q, C.R).chosen[0] == nb[1]
    # a query that is no surface point scans from position 0; every point a query
    mid = K.points((1.0, 2.0, 3.0))
    assert check(ctx, ref, xyz, one, mid, C.R).kmax == 320
    check(ctx, ref, xyz, nrm, xyz, C.R)


def test_order(ctx, ref):
    """A few hundred neighbours with random unit normals: the bits equal the restatement's and differ
    from those of its reversed walk."""
    c = K.order_case()
    want = check(ctx, ref, c["xyz"], c["normals"], c["q"], C.R)
    rev = P.frames(ref, *c["xyz"], *c["normals"], *c["q"], C.R, reversed_order=True)
    assert want.kmax == c["k"] and (bits(want.rf) != bits(rev.rf)).any()


def test_three_tangent_radii_on_one_cloud(ctx, ref):
    """Unset, equal to r (r is a float32 number, so that double(tangent_radius) == r holds), smaller
    and, beyond the issue's three, larger than r (the keys are then gathered at the tangent radius and
    the support is their prefix)."""
    xyz, nrm = K.random_cloud()
    r = float(np.float32(0.05))
    rf = {}
    for tangent_radius in (0.0, r, 0.03, 0.07):
        want = check(ctx, ref, xyz, nrm, xyz, r, tangent_radius)
        assert np.isfinite(want.rf).all(axis=1).sum() > 500
        rf[tangent_radius] = want.rf
    # the radii decide rows: the margin of the equal radius, the smaller set of the smaller one
    assert (bits(rf[0.0]) != bits(rf[r])).any() and (bits(rf[r]) != bits(rf[0.03])).any()
    assert (bits(rf[0.03]) != bits(rf[0.07])).any()
    # z does not depend on the tangent radius: the support is the same
    for tangent_radius in (r, 0.03, 0.07):
        assert np.array_equal(bits(rf[0.0][:, 6:]), bits(rf[tangent_radius][:, 6:]))


# ---- 3. the two passes and the capacity ----

def test_pass_boundary(ctx, ref):
    cap = ctx.stat("board_cap_small")
    assert cap == 2048
    xyz, blobs = E.exact_k_blobs(caps=[cap], deltas=(-1, 0, 1))
    nrm = C.unit_normals(len(xyz[0]), 742)
    qr = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    assert [k for k, _, _ in blobs] == [cap - 1, cap, cap + 1]
    want = check(ctx, ref, xyz, nrm, rows_of(xyz, qr), E.R, queued_rows=3)     # only the blob above the capacity
    assert want.kmax == cap + 1 and np.isfinite(want.rf).all()


def test_second_pass_stride_loop(ctx, ref):
    """One blob of 2,049 points, 600 of them queries: more queued queries than the second pass's 256
    workgroups."""
    xyz, blobs = E.exact_k_blobs(caps=[2048], deltas=(1,))
    (k, lo, hi), = blobs
    nrm = C.unit_normals(len(xyz[0]), 752)
    q = rows_of(xyz, slice(lo, lo + 600))
    assert k == 2049
    want = check(ctx, ref, xyz, nrm, q, E.R, queued_rows=600)
    assert want.neighbors == 600 * 2049


def test_capacity(ctx, ref):
    """16,384 neighbours pass; 16,385 give PFX_ERR_CAPACITY, and the next call is unaffected."""
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(0, 1))
    (k0, lo0, hi0), (k1, lo1, hi1) = blobs
    assert (k0, k1) == (16384, 16385)
    nrm = C.unit_normals(len(xyz[0]), 762)
    q, bad = rows_of(xyz, [lo0, hi0 - 1]), rows_of(xyz, [lo0, lo1])
    want = check(ctx, ref, xyz, nrm, q, E.R, queued_rows=2)
    assert want.kmax == 16384 and np.isfinite(want.rf).all()
    with pytest.raises(PfxError) as e:
        ctx.board_lrf(*xyz, *nrm, *bad, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value) and "16384" in str(e.value)
    same(ctx.board_lrf(*xyz, *nrm, *q, E.R), want.rf, "board frames after the error")


def test_dev_form_reports_a_late_capacity_error_at_synchronize(ref):
    import torch
    from pcl_feature_extraction_amd import Context, PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(1,))
    (k, lo, hi), = blobs
    nrm = C.unit_normals(len(xyz[0]), 772)
    s, sn = up(*xyz), up(*nrm)
    q = up(*rows_of(xyz, [0, lo]))       # the anchor (a lone point) and a point of the blob beyond capacity
    out = torch.zeros((2, 9), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.board_lrf_dev(*s, *sn, *q, E.R, out)     # returns without the error
        with pytest.raises(PfxError) as e:
            c.synchronize()
        assert e.value.code == PFX_ERR_CAPACITY and str(k) in str(e.value)
        c.synchronize()   # reported once
        ok = up(*rows_of(xyz, [0]))
        c.board_lrf_dev(*s, *sn, *ok, E.R, out[:1])   # the next call is unaffected
        c.synchronize()
        assert c.stat("board_kmax") == 1
    assert all_nan(out[:1].cpu().numpy())            # k = 1 < 6


# ---- 4. the reference cloud, and the frames' consumers ----

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
    return dict(xyz=xyz, normals=nrm, q=q, want=P.frames(ref, *xyz, *nrm, *q, 0.08))


def test_reference_cloud_at_its_keypoints(ctx, indoor):
    xyz, nrm, q, want = indoor["xyz"], indoor["normals"], indoor["q"], indoor["want"]
    same(ctx.board_lrf(*xyz, *nrm, *q, 0.08), want.rf, "board frames")
    assert stats(ctx) == (want.neighbors, want.kmax, int((want.k > 2048).sum()))
    assert all_nan(want.rf[-1]) and np.isfinite(want.rf[:-1]).all(axis=1).sum() > 0.95 * len(want.rf)
    assert want.neighbors > 100 * len(want.rf)
    # x and z have unit length and y is z cross x, to float32's precision: 1e-6 covers the cast of a
    # unit double vector (6e-8 a component), a division by a rounded norm (a few 1e-7) and the six
    # products and three differences of a cross product of components below 1 (6e-8 each).  (How far x
    # is from z's plane depends on how close the chosen neighbour lies, and is not a property of
    # the frame's arithmetic.)
    f = want.rf[np.isfinite(want.rf).all(axis=1)].astype(np.float64).reshape(-1, 3, 3)
    assert np.abs(np.linalg.norm(f[:, 0], axis=1) - 1).max() < 1e-6
    assert np.abs(np.linalg.norm(f[:, 2], axis=1) - 1).max() < 1e-6
    assert np.abs(f[:, 1] - np.cross(f[:, 2], f[:, 0])).max() < 1e-6


def test_dev_form_on_a_callers_stream(indoor):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    s, sn, q = up(*indoor["xyz"]), up(*indoor["normals"]), up(*indoor["q"])
    nq = len(indoor["q"][0])
    out = [torch.full((nq, 9), -1.0, dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.set_stream(stream.cuda_stream)
        # no host wait between these launches and synchronize()
        c.board_lrf_dev(*s, *sn, *q, 0.08, out[0])
        c.board_lrf_dev(*s, *sn, *q, 0.08, out[1])
        c.synchronize()
        assert (c.stat("board_neighbors"), c.stat("board_kmax")) == (indoor["want"].neighbors, indoor["want"].kmax)
    for o in out:
        same(o.cpu().numpy(), indoor["want"].rf, "board_lrf_dev")


def test_usc_takes_board_frames(ctx, indoor, tmp_path_factory):
    """ctx.usc with BOARD's rows as its frames, on the rows that have one, equals the USC restatement
    fed with the same frames."""
    sc = SC.build(tmp_path_factory.mktemp("sc_ref"))
    xyz, rf = indoor["xyz"], indoor["want"].rf
    keep = np.flatnonzero(np.isfinite(rf).all(axis=1))[:64]
    q, frames = rows_of(indoor["q"], keep), rf[keep]
    assert len(keep) == 64
    desc, out_rf = ctx.usc(*xyz, *q, frames, 0.08)
    want = SC.usc(sc, *xyz, *q, frames, 0.08)
    same(desc, want.desc, "usc on board frames")
    same(out_rf, want.rf, "usc's rf")
    assert np.array_equal(bits(out_rf), bits(frames)) and np.isfinite(desc).all() and (desc > 0).any(axis=1).all()


def test_correspondences_on_the_x_axes(ctx, indoor, ref):
    """Features<ReferenceFrame>::findCorrespondences compares the first three floats: the mutual
    nearest x axes of two frame sets, against the match model."""
    from pcl_feature_extraction_amd.pcd import read_pcd
    rf = indoor["want"].rf
    src = rf[np.isfinite(rf).all(axis=1)][:200, :3]
    t = read_pcd(os.path.join(CLOUDS, "indoor_target.pcd"))
    txyz = (t.x, t.y, t.z)
    tn = tuple(ctx.normals(*txyz, 0.05)[:3])
    rows = np.arange(0, len(t.x), len(t.x) // 150)[:150]
    trf = ctx.board_lrf(*txyz, *tn, *rows_of(txyz, rows), 0.08)
    same(trf, P.frames(ref, *txyz, *tn, *rows_of(txyz, rows), 0.08).rf, "target frames")
    tgt = trf[np.isfinite(trf).all(axis=1)][:, :3]
    assert len(src) == 200 and len(tgt) > 100
    l2 = M.l2_simple_all(src, tgt)
    s2t, t2s = l2.argmin(axis=1), l2.argmin(axis=0)     # (argmin takes the first minimum)
    mutual = np.flatnonzero(t2s[s2t] == np.arange(len(src)))
    qi, mi = ctx.correspondences(src, tgt)
    assert len(mutual) > 10 and np.array_equal(qi, mutual) and np.array_equal(mi, s2t[mutual])
