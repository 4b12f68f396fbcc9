"""Intensity gradients and RIFT (pfx_intensity_gradient / pfx_rift and their _dev forms, pfx_rift.hip)
against the CPU restatements (tests/cpp/rift_ref.cpp, pinned by tests/test_rift_ref.py): raw bits of
every row of both outputs and every statistic.  Shapes are the smallest that reach every path of the
kernels: wave-edge and chunk-edge neighbourhood sizes, the switch between the two passes at its exact
capacity, the capacity itself, wrapped gradient columns that collide, every tail of the summation
rule."""
import os

import numpy as np
import pytest

import list_edge_clouds as E
import pfh_cases as C
import rift_cases as K
import rift_ref as P
from parity import bits, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = os.path.join(ROOT, "tests", "golden", "clouds")
Z = (0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("rift_ref"))


def rows_of(a, rows):
    return tuple(v[rows] for v in a)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(got)} differ"


def all_nan(rows):
    return (bits(rows) == K.NAN_BITS).all()


def check_gradient(ctx, ref, xyz, inten, q, qn, r=K.R, same_as_surface=False):
    """ctx.intensity_gradient == the restatement, rows and statistics; returns the restatement's result."""
    want = P.gradient(ref, *xyz, inten, *q, *qn, r)
    same(ctx.intensity_gradient(*xyz, inten, *q, *qn, r, same_as_surface=same_as_surface), want.out, "gradient")
    assert (ctx.stat("igrad_neighbors"), ctx.stat("igrad_kmax")) == (want.neighbors, want.kmax)
    return want


def check_rift(ctx, ref, xyz, grads, centres, r=K.R, D=4, G=8):
    want = P.rift(ref, *xyz, *grads, *centres, r, D, G)
    same(ctx.rift(*xyz, *grads, *centres, r, D, G), want.out, "rift")
    assert (ctx.stat("rift_neighbors"), ctx.stat("rift_kmax")) == (want.neighbors, want.kmax)
    return want


# ---- 1. the reference cloud ----

@pytest.fixture(scope="module")
def indoor(ctx, ref):
    """Indoor source: intensities from its colours, normals at 0.05, the whole-cloud gradient at 0.05
    (the restatement's, once), 64 seeded cloud rows + 3 points off the cloud."""
    from pcl_feature_extraction_amd import rgb_to_intensity
    from pcl_feature_extraction_amd.pcd import read_pcd
    c = read_pcd(os.path.join(CLOUDS, "indoor_source.pcd"))
    xyz = (c.x, c.y, c.z)
    inten = rgb_to_intensity(np.ascontiguousarray(c.fields["rgb"]).view(np.uint32))
    nrm = tuple(ctx.normals(*xyz, 0.05)[:3])
    fin = np.flatnonzero(np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.z))
    rows = np.sort(np.random.default_rng(21).choice(fin, 64, replace=False))
    a, b = rows[0], rows[1]
    extra = np.array([[9.0e3, 9.0e3, 9.0e3],                                            # far outside: k = 0
                      [c.x[a] + 0.003, c.y[a] - 0.002, c.z[a] + 0.001],                 # beside a cloud point
                      [c.x[b] - 0.01, c.y[b] + 0.01, c.z[b]]], np.float32)
    q = tuple(np.concatenate([v[rows], extra[:, i]]).astype(np.float32) for i, v in enumerate(xyz))
    qn = tuple(np.concatenate([v[rows], v[[a, a, b]]]).astype(np.float32) for v in nrm)
    cloud = P.gradient(ref, *xyz, inten, *xyz, *nrm, 0.05)
    grads = tuple(np.ascontiguousarray(cloud.out[:, i]) for i in range(3))
    return dict(xyz=xyz, intensity=inten, normals=nrm, rows=rows, q=q, qn=qn, cloud=cloud, grads=grads,
                grad_q=P.gradient(ref, *xyz, inten, *q, *qn, 0.08), rift_q=P.rift(ref, *xyz, *grads, *q, 0.08))


def test_rgb_to_intensity_is_float32_left_to_right():
    from pcl_feature_extraction_amd import rgb_to_intensity
    rgb = np.random.default_rng(3).integers(0, 1 << 24, 4096).astype(np.uint32)
    r, g, b = ((rgb >> s) & 255 for s in (16, 8, 0))
    want = [(np.float32(0.299) * np.float32(x) + np.float32(0.587) * np.float32(y)) + np.float32(0.114) * np.float32(z)
            for x, y, z in zip(r, g, b)]
    got = rgb_to_intensity(rgb)
    assert got.dtype == np.float32 and bits_equal(got, np.float32(want))


def test_whole_cloud_gradient_on_the_reference_cloud(ctx, indoor):
    want = indoor["cloud"]
    got = ctx.intensity_gradient(*indoor["xyz"], indoor["intensity"], *indoor["xyz"], *indoor["normals"], 0.05,
                                 same_as_surface=True)
    same(got, want.out, "whole-cloud gradient")
    assert (ctx.stat("igrad_neighbors"), ctx.stat("igrad_kmax")) == (want.neighbors, want.kmax)
    assert np.isfinite(want.out).all(axis=1).sum() > 0.9 * len(want.out) and want.kmax > 64


def test_both_gradient_paths_agree_on_the_reference_cloud(ctx, indoor):
    rows = indoor["rows"]
    got = ctx.intensity_gradient(*indoor["xyz"], indoor["intensity"], *rows_of(indoor["xyz"], rows),
                                 *rows_of(indoor["normals"], rows), 0.05)
    same(got, indoor["cloud"].out[rows], "query path against the whole-cloud rows")
    assert np.isfinite(got).all(axis=1).sum() > 48


def test_gradient_and_rift_at_queries_on_the_reference_cloud(ctx, indoor):
    xyz, q = indoor["xyz"], indoor["q"]
    want = indoor["grad_q"]
    same(ctx.intensity_gradient(*xyz, indoor["intensity"], *q, *indoor["qn"], 0.08), want.out, "gradient")
    assert (ctx.stat("igrad_neighbors"), ctx.stat("igrad_kmax")) == (want.neighbors, want.kmax)
    assert all_nan(want.out[64]) and np.isfinite(want.out[:64]).all() and want.neighbors > 64 * 100
    want = indoor["rift_q"]
    same(ctx.rift(*xyz, *indoor["grads"], *q, 0.08), want.out, "rift")
    assert (ctx.stat("rift_neighbors"), ctx.stat("rift_kmax"), ctx.stat("rift_queued")) == (want.neighbors, want.kmax, 0)
    assert want.out.shape == (67, 32) and all_nan(want.out[64]) and np.isfinite(want.out[:64]).all(axis=1).sum() > 32


# ---- 2. neighbourhood sizes ----

def test_neighbourhood_sizes_at_wave_and_chunk_edges(ctx, ref):
    ks = (2, 3, 63, 64, 65, 255, 256, 257)
    c = K.blobs_case(ks, 530)
    xyz = c["xyz"]
    qr = np.array([r for lo, hi in c["rows"] for r in sorted(set(E.three_rows(lo, hi)))])
    want = check_gradient(ctx, ref, xyz, c["intensity"], rows_of(xyz, qr), rows_of(c["normals"], qr))
    assert all_nan(want.out[:2]) and np.isfinite(want.out[2:]).all() and want.kmax == 257
    whole = check_gradient(ctx, ref, xyz, c["intensity"], xyz, c["normals"], same_as_surface=True)
    assert bits_equal(whole.out[qr], want.out)
    want = check_rift(ctx, ref, xyz, c["gradients"], rows_of(xyz, qr))
    assert np.isfinite(want.out).all() and want.kmax == 257


def test_pass_boundary(ctx, ref):
    cap = ctx.stat("rift_cap_small")
    xyz, blobs = E.exact_k_blobs(caps=[cap], deltas=(-1, 0, 1))
    n = len(xyz[0])
    inten, grads, nrm = K.intensities(n, 540), K.random_vectors(n, 541, 30.0), C.unit_normals(n, 542)
    qr = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    assert [k for k, _, _ in blobs] == [cap - 1, cap, cap + 1]
    want = check_gradient(ctx, ref, xyz, inten, rows_of(xyz, qr), rows_of(nrm, qr), E.R)
    assert want.kmax == cap + 1 and np.isfinite(want.out).all()
    whole = check_gradient(ctx, ref, xyz, inten, xyz, nrm, E.R, same_as_surface=True)
    assert bits_equal(whole.out[qr], want.out)
    want = check_rift(ctx, ref, xyz, grads, rows_of(xyz, qr), E.R)
    assert want.kmax == cap + 1 and ctx.stat("rift_queued") == 3   # only the blob above the capacity


def test_capacity(ctx, ref):
    """16,384 neighbours pass; 16,385 give PFX_ERR_CAPACITY, and the next call is unaffected."""
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(0, 1))
    (k0, lo0, hi0), (k1, lo1, hi1) = blobs
    assert (k0, k1) == (16384, 16385)
    n = len(xyz[0])
    inten, grads, nrm = K.intensities(n, 550), K.random_vectors(n, 551, 30.0), C.unit_normals(n, 552)
    q, qn = rows_of(xyz, [lo0, hi0 - 1]), rows_of(nrm, [lo0, hi0 - 1])
    bad = rows_of(xyz, [lo0, lo1])
    gw = check_gradient(ctx, ref, xyz, inten, q, qn, E.R)
    assert gw.kmax == 16384
    with pytest.raises(PfxError) as e:
        ctx.intensity_gradient(*xyz, inten, *bad, *qn, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value)
    same(ctx.intensity_gradient(*xyz, inten, *q, *qn, E.R), gw.out, "gradient after the error")
    rw = check_rift(ctx, ref, xyz, grads, q, E.R)
    assert rw.kmax == 16384 and ctx.stat("rift_queued") == 2
    with pytest.raises(PfxError) as e:
        ctx.rift(*xyz, *grads, *bad, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value)
    same(ctx.rift(*xyz, *grads, *q, E.R), rw.out, "rift after the error")


# ---- 3. bin shapes ----

@pytest.mark.parametrize("dg", [(4, 8), (4, 1), (4, 2), (1, 1), (2, 3), (3, 5), (16, 16)])
def test_bin_shapes(ctx, ref, dg):
    """G < 3: the wrapped columns collide and the order within a neighbour decides bits.  D G mod 8 =
    0, 4, 0, 1, 6, 7, 0 with D G = 1 and 4 below the packet pair: the tails of the summation rule."""
    D, G = dg
    c = K.order_case(k=300, blobs=3)
    want = check_rift(ctx, ref, c["xyz"], c["gradients"], c["q"], K.R, D, G)
    assert want.out.shape == (3, D * G) and np.isfinite(want.out).all() and want.neighbors == 900


def test_order(ctx, ref):
    """A few hundred neighbours a row: the bits equal the restatement's, which tests/test_rift_ref.py
    shows to depend on the neighbour order."""
    c = K.order_case()
    check_gradient(ctx, ref, c["xyz"], c["intensity"], c["q"], c["qnormals"])
    check_rift(ctx, ref, c["xyz"], c["gradients"], c["q"])


# ---- 4. the special rows ----

def test_gradient_special_rows(ctx, ref):
    c = K.plane_case()
    xyz, inten, nrm = c["xyz"], c["intensity"], c["normals"]
    want = check_gradient(ctx, ref, xyz, inten, xyz, nrm)
    assert np.abs(want.out - np.float32(c["want"])).max() < 1e-5
    check_gradient(ctx, ref, xyz, inten, xyz, nrm, same_as_surface=True)
    two = K.points(K.Q0, K.offset(K.STEP))
    q = K.points((9.0e3, 9.0e3, 9.0e3), (np.nan, 2.0, 3.0), K.Q0)
    assert all_nan(check_gradient(ctx, ref, two, np.float32([1.0, 2.0]), q, K.vectors(3, Z)).out)   # k = 0, 0, 2
    n = tuple(v.copy() for v in nrm)
    n[0][5] = np.nan
    i2 = inten.copy()
    i2[9] = np.nan
    for ss in (False, True):
        want = check_gradient(ctx, ref, xyz, inten, xyz, n, same_as_surface=ss)          # a NaN normal
        assert all_nan(want.out[5]) and np.isfinite(np.delete(want.out, 5, axis=0)).all()
        assert all_nan(check_gradient(ctx, ref, xyz, i2, xyz, nrm, same_as_surface=ss).out)  # a NaN intensity
    # a non-finite point of the cloud is no neighbour, and as a query it has a NaN row
    x2 = xyz[0].copy()
    x2[3] = np.nan
    for ss in (False, True):
        want = check_gradient(ctx, ref, (x2, xyz[1], xyz[2]), inten, (x2, xyz[1], xyz[2]), nrm, same_as_surface=ss)
        assert all_nan(want.out[3]) and want.kmax == 63
    empty = ctx.intensity_gradient(*xyz, inten, *rows_of(xyz, slice(0, 0)), *rows_of(nrm, slice(0, 0)), K.R)
    assert empty.shape == (0, 3)
    none = ctx.intensity_gradient(*rows_of(xyz, slice(0, 0)), inten[:0], *xyz, *nrm, K.R)   # no surface: every k is 0
    assert all_nan(none) and ctx.stat("igrad_neighbors") == 0


def test_rift_special_rows(ctx, ref):
    q0 = K.points(K.Q0)
    want = check_rift(ctx, ref, q0, K.vectors(1, (0.0, 0.0, 2.0)), q0)       # only itself
    assert want.out[0, 0] == 1.0 and not want.out[0, 1:].any()
    for g in ((3.0, 0.0, 0.0), (-3.0, 0.0, 0.0), (0.0, 0.0, 5.0)):              # parallel, antiparallel, perpendicular
        xyz, grads = K.pair(g)
        assert np.isfinite(check_rift(ctx, ref, xyz, grads, q0).out).all()
    far = K.points((9.0e3, 9.0e3, 9.0e3), (np.nan, 2.0, 3.0))
    assert all_nan(check_rift(ctx, ref, q0, K.vectors(1, (0.0, 0.0, 2.0)), far).out)       # k = 0
    xyz, grads = K.pair((0.0, 0.0, 0.0))
    assert all_nan(check_rift(ctx, ref, xyz, grads, q0).out)                               # all-zero gradients
    xyz, grads = K.pair((1.0, np.nan, 0.0), centre_gradient=(1.0, 2.0, 3.0))
    assert all_nan(check_rift(ctx, ref, xyz, grads, q0).out)                               # a NaN gradient
    # duplicates of the centre and an empty surface
    xyz = K.points(K.Q0, K.Q0, K.offset(K.STEP), K.offset(0.0, -K.STEP))
    check_rift(ctx, ref, xyz, K.random_vectors(4, 560), xyz)
    assert ctx.rift(*xyz, *K.random_vectors(4, 560), *rows_of(xyz, slice(0, 0)), K.R).shape == (0, 32)
    none = ctx.rift(*rows_of(xyz, slice(0, 0)), *rows_of(xyz, slice(0, 0)), *xyz, K.R)
    assert all_nan(none) and ctx.stat("rift_neighbors") == 0


# ---- 5. the _dev forms ----

def test_dev_forms_on_a_callers_stream(indoor):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    s = up(*indoor["xyz"])
    si, = up(indoor["intensity"])
    sn, sg, q, qn = up(*indoor["normals"]), up(*indoor["grads"]), up(*indoor["q"]), up(*indoor["qn"])
    nq, ns = len(indoor["q"][0]), len(indoor["xyz"][0])
    g_q = [torch.full((nq, 3), -1.0, dtype=torch.float32, device=dev) for _ in range(2)]
    g_all = torch.full((ns, 3), -1.0, dtype=torch.float32, device=dev)
    r_q = [torch.full((nq, 32), -1.0, dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.set_stream(stream.cuda_stream)
        # no host wait between these launches and synchronize()
        c.intensity_gradient_dev(*s, si, *q, *qn, 0.08, g_q[0])
        c.rift_dev(*s, *sg, *q, 0.08, r_q[0])
        c.intensity_gradient_dev(*s, si, *q, *qn, 0.08, g_q[1])
        c.rift_dev(*s, *sg, *q, 0.08, r_q[1])
        c.synchronize()
        for what, want in (("igrad", indoor["grad_q"]), ("rift", indoor["rift_q"])):
            assert (c.stat(what + "_neighbors"), c.stat(what + "_kmax")) == (want.neighbors, want.kmax)
        c.trim()
        c.intensity_gradient_dev(*s, si, *s, *sn, 0.05, g_all, same_as_surface=True)
        c.synchronize()
        assert (c.stat("igrad_neighbors"), c.stat("igrad_kmax")) == (indoor["cloud"].neighbors, indoor["cloud"].kmax)
    for o in g_q:
        same(o.cpu().numpy(), indoor["grad_q"].out, "gradient_dev")
    for o in r_q:
        same(o.cpu().numpy(), indoor["rift_q"].out, "rift_dev")
    same(g_all.cpu().numpy(), indoor["cloud"].out, "whole-cloud gradient_dev")


def test_dev_forms_report_a_late_capacity_error_at_synchronize(ref):
    import torch
    from pcl_feature_extraction_amd import Context, PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(1,))
    (k, lo, hi), = blobs
    n = len(xyz[0])
    inten, grads, nrm = K.intensities(n, 570), K.random_vectors(n, 571, 30.0), C.unit_normals(n, 572)
    rows = [0, lo]       # the anchor (a lone point) and a point of the blob beyond capacity
    s, (si,), sg = up(*xyz), up(inten), up(*grads)
    q, qn = up(*rows_of(xyz, rows)), up(*rows_of(nrm, rows))
    out_g = torch.zeros((2, 3), dtype=torch.float32, device=dev)
    out_r = torch.zeros((2, 32), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        for launch in (lambda: c.intensity_gradient_dev(*s, si, *q, *qn, E.R, out_g),
                       lambda: c.rift_dev(*s, *sg, *q, E.R, out_r)):
            launch()     # returns without the error
            with pytest.raises(PfxError) as e:
                c.synchronize()
            assert e.value.code == PFX_ERR_CAPACITY and str(k) in str(e.value)
            c.synchronize()   # reported once
        # the next call is unaffected
        ok = up(*rows_of(xyz, [0]))
        c.rift_dev(*s, *sg, *ok, E.R, out_r[:1])
        c.synchronize()
        want = P.rift(ref, *xyz, *grads, *rows_of(xyz, [0]), E.R)
        assert c.stat("rift_kmax") == want.kmax == 1
    same(out_r[:1].cpu().numpy(), want.out, "rift_dev after the error")


# ---- 6. invalid arguments ----

def test_invalid_arguments(ctx):
    import ctypes
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID
    c = K.order_case(k=8, blobs=1)
    xyz, inten, grads, nrm = c["xyz"], c["intensity"], c["gradients"], c["normals"]
    ctx.rift(*xyz, *grads, *xyz, K.R)
    ctx.intensity_gradient(*xyz, inten, *xyz, *nrm, K.R)
    before = ctx.stat("rift_kmax"), ctx.stat("igrad_kmax")
    assert before == (8, 8)
    for kw in (dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(D=0), dict(D=17), dict(G=0), dict(G=17)):
        with pytest.raises(PfxError) as e:
            ctx.rift(*xyz, *grads, *xyz, kw.get("r", K.R), kw.get("D", 4), kw.get("G", 8))
        assert e.value.code == PFX_ERR_INVALID, kw
    for r in (0.0, float("nan")):
        with pytest.raises(PfxError) as e:
            ctx.intensity_gradient(*xyz, inten, *xyz, *nrm, r)
        assert e.value.code == PFX_ERR_INVALID
    with pytest.raises(PfxError) as e:   # same_as_surface with other queries
        ctx.intensity_gradient(*xyz, inten, *rows_of(xyz, slice(0, 4)), *rows_of(nrm, slice(0, 4)), K.R,
                               same_as_surface=True)
    assert e.value.code == PFX_ERR_INVALID
    # null pointers, straight at the C-ABI
    lib, p = ctx._lib, lambda v: v.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = np.empty((8, 32), np.float32)
    a = [p(v) for v in (*xyz, *grads)] + [8] + [p(v) for v in xyz] + [8, K.R, 4, 8, p(out)]
    for null in (0, 3, 8, 14):
        b = list(a)
        b[null] = None
        assert lib.pfx_rift(ctx.h, *b) == PFX_ERR_INVALID
    a = [p(v) for v in (*xyz, inten)] + [8] + [p(v) for v in (*xyz, *nrm)] + [8, 0, K.R, p(out)]
    for null in (0, 3, 5, 8, 14):
        b = list(a)
        b[null] = None
        assert lib.pfx_intensity_gradient(ctx.h, *b) == PFX_ERR_INVALID
    # nothing was launched: the statistics are those of the last valid calls, and the context works
    assert (ctx.stat("rift_kmax"), ctx.stat("igrad_kmax")) == before
    assert np.isfinite(ctx.rift(*xyz, *grads, *xyz, K.R)).all()
