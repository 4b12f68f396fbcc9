"""NARF descriptors (pfx_narf_descriptors and its _dev form, pfx_narf_desc.hip) and the point indices
(pfx_point_indices) against the CPU restatement (tests/cpp/narf_desc_ref.cpp, pinned by
tests/test_narf_desc_ref.py): descriptors, poses, row keys, the row count and all six statistics, bit
for bit, no row excluded.  Each case first shows on the restatement alone that it reaches what it is
there for."""
import numpy as np
import pytest

import narf_desc_cases as K
import narf_desc_ref as P
import oracle_lib as O
from pcl_feature_extraction_amd import camera, narf_desc_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("narf_desc_ref"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stats(ctx):
    return {s: ctx.stat("narf_desc_" + s) for s in P.STATS}


def same(got, want, what):
    assert got.desc.shape == want.desc.shape and got.pose.shape == want.pose.shape, what
    assert np.array_equal(got.keypoint, want.keypoint), what
    for name in ("desc", "pose"):
        g, w = bits(getattr(got, name)), bits(getattr(want, name))
        bad = np.flatnonzero((g != w).any(axis=1))
        assert len(bad) == 0, (f"{what}: {name} rows {bad[:8].tolist()} of {len(g)} differ; the first: "
                               f"{getattr(got, name)[bad[0]].tolist()} for {getattr(want, name)[bad[0]].tolist()}")


def nonvacuous(want, nk, reach):
    s = want.stats
    per = np.bincount(want.keypoint, minlength=nk)
    assert s["rows"] == len(want.desc) > 0 and s["invalid_pixels"] > 0
    if "multi" in reach:
        assert (per >= 2).sum() >= 3
    if "fallback" in reach:
        assert s["fallback_normals"] > 0
    if "failed" in reach:
        assert s["pose_failed"] > 0
    else:
        assert s["ring_max"] > 64 // 8  # (a ring of more than one 64-position chunk)
    if "background" in reach:
        assert s["background_cells"] > 0
    if "rings" in reach:
        assert s["ring_max"] >= 40  # 320 positions and more: five chunks


def rings_leave_the_image_on_all_four_sides(ref, x, y, z, cam, pix, support):
    """(on the restatement alone) for each border, the valid entry nearest to it, run by itself: its
    largest ring reaches beyond that border, and is one of several 64-position chunks."""
    w, h = cam["width"], cam["height"]
    valid = np.isfinite(O.range_image_planar(x, y, z, cam=cam)[..., 3].ravel())
    p = pix[(pix >= 0) & (pix < w * h)]
    p = p[valid[p]]
    px, py = p % w, p // w
    for side, entry in (("left", p[px.argmin()]), ("right", p[px.argmax()]), ("top", p[py.argmin()]),
                        ("bottom", p[py.argmax()])):
        one = P.descriptors(ref, x, y, z, [entry], support, True, cam)
        r, ex, ey = one.stats["ring_max"], int(entry) % w, int(entry) // w
        assert one.stats["invalid_pixels"] == 0 and 8 * r > 2 * 64, side
        assert {"left": ex - r < 0, "right": ex + r >= w, "top": ey - r < 0, "bottom": ey + r >= h}[side], (side, ex, ey, r)


@pytest.mark.parametrize("name,support,rotinv,reach", K.GPU_CASES,
                         ids=["%s-%g-%s" % (c[0], c[1], "inv" if c[2] else "plain") for c in K.GPU_CASES])
def test_kernel_gives_the_restatements_bits(ctx, ref, name, support, rotinv, reach):
    x, y, z, cam, pix = K.indoor(name)
    want = P.descriptors(ref, x, y, z, pix, support, rotinv, cam)
    nonvacuous(want, len(pix), reach)
    if (name, support) == ("S", 1.0):
        rings_leave_the_image_on_all_four_sides(ref, x, y, z, cam, pix, support)
    if name == "full":
        assert len(pix) <= 64 and pix.max() >= 640 * 480 - 1
    got = ctx.narf_descriptors(x, y, z, pix, narf_desc_params(support, rotinv), camera(**cam))
    same(got, want, name)
    assert stats(ctx) == want.stats


@pytest.mark.parametrize("scene", ["x_ridge", "square_far", "square_alone", "groove"])
def test_synthetic_scenes_as_clouds(ctx, ref, scene):
    """The scenes of test_narf_desc_ref.py as clouds (every pixel's point projects back onto its pixel):
    four rotations, the 48 background cells and none, the step."""
    depth = {"x_ridge": lambda: K.relief_depth(K.x_ridge), "square_far": lambda: K.square_depth(3.0),
             "square_alone": lambda: K.square_depth(np.nan), "groove": K.groove_depth}[scene]()
    x, y, z = K.image_cloud(K.depth_image(depth, K.Q))
    pix = np.array([K.Q_CENTRE, K.Q_CENTRE - 3 * 65 + 2, 0], np.int32)
    for rotinv in (True, False):
        want = P.descriptors(ref, x, y, z, pix, 0.2, rotinv, K.Q)
        if scene == "x_ridge" and rotinv:
            assert np.bincount(want.keypoint)[0] == 4
        if scene.startswith("square"):
            assert (want.stats["background_cells"] > 0) == (scene == "square_far")
        same(ctx.narf_descriptors(x, y, z, pix, narf_desc_params(0.2, rotinv), camera(**K.Q)), want, scene)
        assert stats(ctx) == want.stats


@pytest.mark.parametrize("nk", [1, 63, 64, 65])
def test_entry_counts_around_a_wave(ctx, ref, nk):
    x, y, z, cam, pix = K.indoor("S")
    ri_valid = O.range_image_planar(x, y, z, cam=cam)[..., 3].ravel()
    pix = pix[(pix >= 0) & (pix < len(ri_valid))]
    pix = pix[np.isfinite(ri_valid[pix])][5:5 + nk]
    want = P.descriptors(ref, x, y, z, pix, 0.2, True, cam)
    assert len(pix) == nk and len(want.desc) >= nk and want.stats["invalid_pixels"] == 0
    same(ctx.narf_descriptors(x, y, z, pix, narf_desc_params(0.2), camera(**cam)), want, nk)
    assert stats(ctx) == want.stats


def test_device_form_and_its_capacity(ctx, ref):
    """cap below the row count: the first cap rows and the full count; at the count: all rows."""
    import torch
    x, y, z, cam, pix = K.indoor("S")
    want = P.descriptors(ref, x, y, z, pix, 0.2, True, cam)
    m = len(want.desc)
    dev = torch.device("cuda", 0)
    dx, dy, dz = (torch.tensor(np.asarray(v), device=dev) for v in (x, y, z))
    dpix = torch.tensor(np.asarray(pix), device=dev)
    for cap in (m - 7, m):
        desc = torch.full((cap, 36), 7.0, device=dev)
        pose = torch.full((cap, 12), 7.0, device=dev)
        key = torch.full((cap,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # (the context runs on its own stream)
        count = ctx.narf_descriptors_dev(dx, dy, dz, dpix, desc, pose, key, narf_desc_params(0.2), camera(**cam))
        ctx.synchronize()
        assert int(count.item()) == m
        assert np.array_equal(bits(desc.cpu().numpy()), bits(want.desc[:cap]))
        assert np.array_equal(bits(pose.cpu().numpy()), bits(want.pose[:cap]))
        assert np.array_equal(key.cpu().numpy(), want.keypoint[:cap])
        assert stats(ctx) == want.stats


def test_point_indices(ctx, ref):
    """The indoor cloud with its Harris keypoints (cloud points: each finds itself, and its duplicates),
    then keypoints beside a cloud point by just under and just over the tolerance, a NaN, and one
    far from everything."""
    x, y, z, _, _ = K.indoor("S")
    x, y, z = (np.concatenate([v, v[100:103]]) for v in (x, y, z))  # three points twice
    kp = ctx.harris3d_keypoints(x, y, z, radius=0.05, threshold=1e-6)
    kp = np.unique(np.concatenate([kp[:200], [100, 101, 102]]))
    kx, ky, kz = x[kp].copy(), y[kp].copy(), z[kp].copy()
    extra = np.array([[x[7] + 0.5e-4, y[7], z[7]], [x[8], y[8] - 2e-4, z[8]], [np.nan, y[9], z[9]], [50.0, 50.0, 50.0]],
                     np.float32)
    kx, ky, kz = (np.concatenate([a, extra[:, i]]) for i, a in enumerate((kx, ky, kz)))
    want = P.point_indices(ref, x, y, z, kx, ky, kz)
    assert len(want) >= len(kp) + 3 + 1 and 7 in want.tolist()
    got = ctx.point_indices(x, y, z, kx, ky, kz)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # more keypoints than a wave and a cloud that is no multiple of the tile
    sel = np.arange(0, len(x), 97)
    want = P.point_indices(ref, x[:5001], y[:5001], z[:5001], x[sel], y[sel], z[sel])
    assert len(sel) > 64 and 0 < len(want) < len(sel)
    assert np.array_equal(ctx.point_indices(x[:5001], y[:5001], z[:5001], x[sel], y[sel], z[sel]), want)


def test_point_indices_device_form(ctx, ref):
    import torch
    x, y, z, _, _ = K.indoor("S")
    sel = np.arange(3, len(x), 501)
    want = P.point_indices(ref, x, y, z, x[sel], y[sel], z[sel])
    dev = torch.device("cuda", 0)
    d = [torch.tensor(np.asarray(v), device=dev) for v in (x, y, z, x[sel], y[sel], z[sel])]
    for cap in (len(want) - 3, len(want)):
        out = torch.full((cap,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # (the context runs on its own stream)
        count = ctx.point_indices_dev(*d, out)
        ctx.synchronize()
        assert int(count.item()) == len(want) and np.array_equal(out.cpu().numpy(), want[:cap])
