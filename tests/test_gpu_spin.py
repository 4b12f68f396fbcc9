"""Spin images (pfx_spin_image / pfx_spin_image_dev, pfx_spin.hip) against the CPU restatement of
PCL 1.7 SpinImageEstimation (tests/cpp/spin_ref.cpp, pinned by tests/test_spin_ref.py): raw bits of
every row, of the double matrix before normalisation and of its sum, and every statistic.  Shapes
are the smallest that reach every path of the kernel: wave-edge and chunk-edge neighbourhood sizes,
the switch between the two passes at its exact capacity, the capacity itself, every tail of the
summation rule."""
import os

import numpy as np
import pytest

import list_edge_clouds as E
import pfh_cases as C
import spin_cases as K
import spin_ref as P
from parity import bits, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = os.path.join(ROOT, "tests", "golden", "clouds")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("spin_ref"))


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rows_of(a, rows):
    return tuple(v[rows] for v in a)


def same(got, want):
    """out, raw and sums of the GPU == the restatement's, bit for bit."""
    out, raw, sums = got
    assert out.shape == want.out.shape and raw.shape == want.raw.shape and sums.shape == want.sums.shape
    bad = np.flatnonzero((bits(out) != bits(want.out)).any(axis=1))
    assert len(bad) == 0, f"out: rows {bad[:8].tolist()} of {len(out)} differ"
    bad = np.flatnonzero((bits64(raw) != bits64(want.raw)).any(axis=1))
    assert len(bad) == 0, f"raw: rows {bad[:8].tolist()} of {len(raw)} differ"
    bad = np.flatnonzero(bits64(sums) != bits64(want.sums))
    assert len(bad) == 0, f"sums: rows {bad[:8].tolist()} of {len(sums)} differ"


def stats_match(ctx, want):
    assert ctx.stat("spin_neighbors") == want.neighbors and ctx.stat("spin_kmax") == want.kmax
    assert ctx.stat("spin_too_few") == want.too_few and ctx.stat("spin_bad_cos") == want.bad_cos


def check(ctx, ref, xyz, q, axes, r=K.R, **kw):
    """ctx.spin_image == the restatement (no offending row expected); returns the restatement's result."""
    want = P.spin(ref, *xyz, *q, *axes, r, **kw)
    assert want.too_few == 0 and want.bad_cos == 0
    same(ctx.spin_image(*xyz, *q, *axes, r, debug=True, **kw), want)
    stats_match(ctx, want)
    return want


@pytest.fixture(scope="module")
def indoor(ctx, ref):
    """Case 1, shared: indoor source, normals at 0.05, 64 seeded cloud rows (their own normals the
    axes) + 3 other points."""
    from pcl_feature_extraction_amd.pcd import read_pcd
    c = read_pcd(os.path.join(CLOUDS, "indoor_source.pcd"))
    xyz = (c.x, c.y, c.z)
    nrm = ctx.normals(*xyz, 0.05)[:3]
    fin = np.flatnonzero(np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.z))
    rows = np.sort(np.random.default_rng(11).choice(fin, 64, replace=False))
    a, b = rows[0], rows[1]
    extra = np.array([[9.0e3, 9.0e3, 9.0e3],                                            # far outside: k = 0
                      [c.x[a] + 0.003, c.y[a] - 0.002, c.z[a] + 0.001],                 # beside a cloud point
                      [c.x[b] - 0.01, c.y[b] + 0.01, c.z[b]]], np.float32)
    q = tuple(np.concatenate([v[rows], extra[:, i]]).astype(np.float32) for i, v in enumerate(xyz))
    axes = tuple(np.concatenate([v[rows], v[[a, a, b]]]).astype(np.float32) for v in nrm)
    return dict(xyz=xyz, q=q, axes=axes, want=P.spin(ref, *xyz, *q, *axes, 0.08))


def test_reference_cloud(ctx, indoor):
    want = indoor["want"]
    same(ctx.spin_image(*indoor["xyz"], *indoor["q"], *indoor["axes"], 0.08, debug=True), want)
    stats_match(ctx, want)
    assert want.out.shape == (67, 153) and want.neighbors > 64 * 100 and want.too_few == want.bad_cos == 0
    assert not want.out[64].any() and want.out[:64].any(axis=1).all()
    assert bits_equal(ctx.spin_image(*indoor["xyz"], *indoor["q"], *indoor["axes"], 0.08), want.out)


def test_axes_from_the_sparse_query_cloud(ctx, ref, indoor):
    """The reference's own usage: the axes are the normals of the query cloud among itself at 0.05,
    mostly NaN.  Such a row is finite and has mass in alpha_bin 0 only."""
    q = indoor["q"]
    axes = ctx.normals(*q, 0.05)[:3]
    nan = np.isnan(axes[0])
    assert nan.sum() > 32
    want = check(ctx, ref, indoor["xyz"], q, axes, 0.08)
    img = want.out.reshape(-1, 9, 17)
    assert np.isfinite(img[nan]).all() and not img[nan][:, 1:].any()
    assert img[nan][:, 0].any(axis=1).sum() > 32


def test_neighbourhood_sizes_at_wave_and_chunk_edges(ctx, ref):
    chunk = ctx.stat("spin_chunk")
    ks = (1, 2, 3, 63, 64, 65, chunk - 1, chunk, chunk + 1)
    xyz, _, rows = C.concat([C.blob(k, (1.0 + s, 2.0, 3.0), 130 + 2 * s) for s, k in enumerate(ks)])
    qr = np.array([r for lo, hi in rows for r in sorted(set(E.three_rows(lo, hi)))])
    want = check(ctx, ref, xyz, rows_of(xyz, qr), C.unit_normals(len(qr), 129))
    assert not want.out[0].any() and want.kmax == chunk + 1                 # k = 1: zeros, not NaN
    assert want.neighbors == sum(k * len(set(E.three_rows(lo, hi))) for k, (lo, hi) in zip(ks, rows))


def test_pass_boundary(ctx, ref):
    cap = ctx.stat("spin_cap_small")
    xyz, blobs = E.exact_k_blobs(caps=[cap], deltas=(-1, 0, 1))
    qr = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    want = check(ctx, ref, xyz, rows_of(xyz, qr), C.unit_normals(len(qr), 141), E.R)
    assert [k for k, _, _ in blobs] == [cap - 1, cap, cap + 1] and want.kmax == cap + 1
    assert ctx.stat("spin_queued") == 3   # only the blob above the capacity takes the second pass


def test_capacity(ctx, ref):
    """16,384 neighbours pass; 16,385 give PFX_ERR_CAPACITY, and the next call is unaffected."""
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    xyz, blobs = E.exact_k_blobs(caps=[16384], deltas=(0, 1))
    (k0, lo0, hi0), (k1, lo1, hi1) = blobs
    assert (k0, k1) == (16384, 16385)
    axes = C.unit_normals(2, 151)
    q = rows_of(xyz, [lo0, hi0 - 1])
    want = check(ctx, ref, xyz, q, axes, E.R)
    assert want.kmax == 16384 and ctx.stat("spin_queued") == 2
    with pytest.raises(PfxError) as e:
        ctx.spin_image(*xyz, *rows_of(xyz, [lo0, lo1]), *axes, E.R)
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value)
    same(ctx.spin_image(*xyz, *q, *axes, E.R, debug=True), want)


def test_order(ctx, ref):
    """A few hundred neighbours a row: raw and sums equal the restatement's bits, which
    tests/test_spin_ref.py shows to depend on the neighbour order and on the summation order."""
    c = K.order_case()
    want = check(ctx, ref, c["xyz"], c["q"], c["axes"])
    assert want.neighbors == 8 * c["k"]


@pytest.mark.parametrize("w", [1, 5, 8, 16, 2, 3])
def test_widths(ctx, ref, w):
    """(W + 1)(2W + 1) mod 4 = 2, 2, 1, 1, 3, 0: every tail of the summation rule, and up to three
    bins a thread."""
    xyz, _ = C.blob(40, K.Q0, 160)
    want = check(ctx, ref, xyz, xyz, C.unit_normals(40, 161), image_width=w)
    assert want.out.shape == (40, (w + 1) * (2 * w + 1)) and want.out.any(axis=1).all()


def test_support_angle(ctx, ref):
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID
    xyz, nrm, kept = K.support_case()
    n = len(xyz[0])
    want = check(ctx, ref, xyz, xyz, K.axes(n), support_angle_cos=0.5, surface_normals=nrm)
    # the query at Q0 sees exactly the kept neighbours
    only = P.spin(ref, *rows_of(xyz, kept), *K.points(K.Q0), *K.axes(1), K.R)
    assert np.array_equal(bits64(want.raw[0]), bits64(only.raw[0]))
    with pytest.raises(PfxError) as e:
        ctx.spin_image(*xyz, *xyz, *K.axes(n), K.R, support_angle_cos=0.5)
    assert e.value.code == PFX_ERR_INVALID


def test_degenerates(ctx, ref):
    (x, y, z), _ = C.blob(48, K.Q0, 170)
    dup = np.arange(0, 48, 6)  # exact duplicates of 8 points
    x, y, z = (np.concatenate([v, v[dup], np.float32([t] * 3)]) for v, t in zip((x, y, z), (7.0, 8.0, 9.0)))
    n = len(x)                 # ... and three copies of one far point: an all-duplicates neighbourhood
    qx, qy, qz = (np.concatenate([v, np.float32([np.nan])]) for v in (x, y, z))
    qy[-1] = 2.0
    want = check(ctx, ref, (x, y, z), (qx, qy, qz), C.unit_normals(n + 1, 171))
    assert np.isnan(want.out[n - 3:n]).all() and not want.sums[n - 3:n].any()
    assert not want.out[n].any() and np.isfinite(want.out[:n - 3]).all()
    empty = ctx.spin_image(x, y, z, x[:0], y[:0], z[:0], x[:0], y[:0], z[:0], K.R)
    assert empty.shape == (0, 153) and empty.dtype == np.float32
    # no surface at all: every k is 0
    none = ctx.spin_image(x[:0], y[:0], z[:0], x, y, z, x, y, z, K.R, debug=True)
    assert not none[0].any() and not none[1].any() and not none[2].any() and ctx.stat("spin_neighbors") == 0


def test_invalid_arguments(ctx):
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID, PFX_ERR_UNSUPPORTED
    xyz, nrm = C.blob(8, K.Q0, 180)
    for kw, code in ((dict(r=0.0), PFX_ERR_INVALID), (dict(image_width=0), PFX_ERR_INVALID),
                     (dict(image_width=17), PFX_ERR_INVALID), (dict(radial=1), PFX_ERR_UNSUPPORTED),
                     (dict(angular=1), PFX_ERR_UNSUPPORTED), (dict(support_angle_cos=1.5), PFX_ERR_INVALID),
                     (dict(support_angle_cos=float("nan")), PFX_ERR_INVALID), (dict(min_pts_neighb=-1), PFX_ERR_INVALID)):
        kw = dict(kw)
        with pytest.raises(PfxError) as e:
            ctx.spin_image(*xyz, *xyz, *nrm, kw.pop("r", K.R), **kw)
        assert e.value.code == code, kw
    assert np.isfinite(ctx.spin_image(*xyz, *xyz, *nrm, K.R)).all()


def test_errors_where_pcl_throws(ctx, ref):
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), 190 + 2 * s) for s, k in enumerate((12, 5, 12))]
    xyz, _, rows = C.concat(parts)
    n = len(xyz[0])
    axes = tuple(v.copy() for v in C.unit_normals(n, 189))
    # too few: the rows of the 5-point blob, the first of them row 12
    want = P.spin(ref, *xyz, *xyz, *axes, K.R, min_pts_neighb=6)
    assert (want.too_few, want.first_few, want.bad_cos) == (5, 12, 0)
    with pytest.raises(PfxError) as e:
        ctx.spin_image(*xyz, *xyz, *axes, K.R, min_pts_neighb=6)
    assert e.value.code == PFX_ERR_INVALID and "row 12 " in str(e.value) and "too few" in str(e.value)
    stats_match(ctx, want)
    # a cosine out of range: an axis of length 1.01 along a neighbour direction, in rows 20 and 3
    for row, nb in ((20, 21), (3, 4)):
        d = np.array([v[nb] - v[row] for v in xyz], np.float64)
        for a, t in zip(axes, 1.01 * d / np.linalg.norm(d)):
            a[row] = t
    want = P.spin(ref, *xyz, *xyz, *axes, K.R)
    assert (want.too_few, want.bad_cos, want.first_bad) == (0, 2, 3)
    with pytest.raises(PfxError) as e:
        ctx.spin_image(*xyz, *xyz, *axes, K.R)
    assert e.value.code == PFX_ERR_INVALID and "row 3 " in str(e.value) and "cosine" in str(e.value)
    stats_match(ctx, want)
    # the context is usable afterwards, and nothing of the errors sticks
    good = [r for r in range(n) if r not in (3, 20)]
    check(ctx, ref, xyz, rows_of(xyz, good), rows_of(axes, good))


def test_spin_image_dev_stream_ordered_and_deterministic(indoor):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
         for a in (*indoor["xyz"], *indoor["q"], *indoor["axes"])]
    want = indoor["want"]
    nq = len(indoor["q"][0])
    outs = [torch.full((nq, 153), -1.0, dtype=torch.float32, device=dev) for _ in range(3)]
    raw = torch.full((nq, 153), -1.0, dtype=torch.float64, device=dev)
    sums = torch.full((nq,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()  # (the context runs on its own stream)
    with Context(0) as c:
        c.spin_image_dev(*t, 0.08, outs[0])
        c.spin_image_dev(*t, 0.08, outs[1], raw=raw, sums=sums)
        c.synchronize()
        c.trim()
        c.spin_image_dev(*t, 0.08, outs[2])
        c.synchronize()
        stats_match(c, want)
    for o in outs:
        assert bits_equal(o.cpu().numpy(), want.out)
    assert np.array_equal(bits64(raw.cpu().numpy()), bits64(want.raw))
    assert np.array_equal(bits64(sums.cpu().numpy()), bits64(want.sums))


def test_matching_at_dim_153(ctx, indoor):
    import oracle_lib as O
    from pcl_feature_extraction_amd.pcd import read_pcd
    t = read_pcd(os.path.join(CLOUDS, "indoor_target.pcd"))
    txyz = (t.x, t.y, t.z)
    tn = ctx.normals(*txyz, 0.05)[:3]
    fin = np.flatnonzero(np.isfinite(t.x) & np.isfinite(t.y) & np.isfinite(t.z))
    rows = np.sort(np.random.default_rng(12).choice(fin, 64, replace=False))
    tgt = ctx.spin_image(*txyz, *rows_of(txyz, rows), *rows_of(tn, rows), 0.08)
    src = indoor["want"].out[:64]
    assert not np.isnan(tgt).any() and not np.isnan(src).any()
    q, m = ctx.correspondences(src, tgt)
    oq, om = O.correspondences(src, tgt)
    assert np.array_equal(q, oq) and np.array_equal(m, om) and len(q) > 0
