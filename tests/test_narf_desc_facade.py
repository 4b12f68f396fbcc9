"""NarfDescriptor of the C++ facade (include/pfx_pcl.hpp): tests/cpp/narf_desc_facade_driver.cpp makes
the calls of the reference's DESC_NARF branch (evaluation.cpp:613-648) up to findCorrespondences
against it, with Tools::getIndices served by pfx_point_indices.  CPU: the driver compiles and links
against libpfx.so.  GPU: the indices are Context.point_indices', the Narf36 rows hold
Context.narf_descriptors' descriptors behind the position and Euler angles of the inverse pose, both
clouds' rows are taken on the SOURCE range image with cloud indices as pixel indices (the branch as
written), the matcher compares the 36 descriptor floats (offset 6 of 42), and a compute() without an
image, indices or a support size fails loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narf_desc_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("narf_desc_facade") / "narf_desc_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_narf_desc_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


def test_facade_declares_the_classes():
    hpp = open(os.path.join(ROOT, "include", "pfx_pcl.hpp")).read()
    assert "class NarfDescriptor {" in hpp and "struct Narf36 {" in hpp
    assert "explicit NarfDescriptor(const RangeImage* range_image = nullptr, const std::vector<int>* indices = nullptr)" in hpp
    assert "DescriptorLayout<Narf36> { static constexpr int dim = 36, stride = 42, offset = 6; };" in hpp
    assert "struct LayoutOffset { static constexpr int value = 0; };" in hpp  # the offset defaults to 0
    # the existing layouts keep their values
    assert "DescriptorLayout<SHOT352> { static constexpr int dim = 352, stride = 361; };" in hpp
    assert "DescriptorLayout<FPFHSignature33> { static constexpr int dim = 33, stride = 33; };" in hpp


def euler_rows(res):
    """x, y, z, roll, pitch, yaw of the inverse of every pose, then the descriptor: (m, 42)."""
    a = res.pose.reshape(-1, 3, 4).astype(np.float32)
    r, t = a[:, :, :3], a[:, :, 3]
    pos = -((r[:, 0, :] * t[:, :1] + r[:, 1, :] * t[:, 1:2]) + r[:, 2, :] * t[:, 2:3])
    m = r.transpose(0, 2, 1)  # the inverse's rotation
    ang = np.stack([np.arctan2(m[:, 2, 1], m[:, 2, 2]), np.arcsin(-m[:, 2, 0]), np.arctan2(m[:, 1, 0], m[:, 0, 0])], 1)
    return np.concatenate([pos, ang.astype(np.float32), res.desc], 1)


@pytest.mark.gpu
def test_narf_desc_facade_matches_c_abi(ctx, driver, tmp_path):
    from pcl_feature_extraction_amd import narf_desc_params
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    src = read_pcd(PCD)
    rows = {}
    for tag, path in (("src", PCD), ("tgt", PCD_T)):
        c = read_pcd(path)
        kp = np.fromfile(tmp_path / f"{tag}_kp_xyz.f32", np.float32).reshape(-1, 3)
        assert len(kp) >= 5  # (the keypoints whose pixel index is also a cloud index)
        idx = np.fromfile(tmp_path / f"{tag}_idx.i32", np.int32)
        want_idx = ctx.point_indices(c.x, c.y, c.z, kp[:, 0], kp[:, 1], kp[:, 2])
        assert len(idx) >= len(kp) and np.array_equal(idx, want_idx), tag
        # cloud indices as pixel indices, on the SOURCE cloud's range image for both
        want = ctx.narf_descriptors(src.x, src.y, src.z, idx, narf_desc_params(0.2, True))
        got = np.fromfile(tmp_path / f"{tag}_rows.f32", np.float32).reshape(-1, 42)
        keys = np.fromfile(tmp_path / f"{tag}_keys.i32", np.int32)
        assert len(want.desc) > 0 and np.array_equal(keys, want.keypoint), tag
        assert np.array_equal(got[:, 6:].view(np.uint32), want.desc.view(np.uint32)), tag
        model = euler_rows(want)
        assert np.array_equal(got[:, :3].view(np.uint32), model[:, :3].view(np.uint32)), tag
        assert np.abs(got[:, 3:6] - model[:, 3:6]).max() < 1e-6, tag  # (libm's atan2f / asinf against numpy's)
        rows[tag] = got
    # the matcher: mutual nearest neighbours over the 36 descriptor floats alone
    corr = np.fromfile(tmp_path / "corr.i32", np.int32).reshape(-1, 2)
    s, t = rows["src"][:, 6:].astype(np.float64), rows["tgt"][:, 6:].astype(np.float64)
    d2 = ((s[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    s2t, t2s = d2.argmin(1), d2.argmin(0)
    want_corr = {(i, int(j)) for i, j in enumerate(s2t) if t2s[j] == i}
    # float64 here against the matcher's float32: a row or column whose two best distances are within
    # 1e-9 of each other (two identical rows, say) may be decided either way, and only the pairs that
    # touch such a row or column are left out of the comparison
    tie_s = np.sort(d2, 1)[:, 1] - np.sort(d2, 1)[:, 0] < 1e-9
    tie_t = np.sort(d2, 0)[1, :] - np.sort(d2, 0)[0, :] < 1e-9
    safe = lambda pairs: {(i, j) for i, j in pairs if not tie_s[i] and not tie_t[j]}  # noqa: E731
    got_corr = {(int(i), int(j)) for i, j in corr}
    assert len(safe(want_corr)) >= 1 and safe(got_corr) == safe(want_corr)
    checks = np.fromfile(tmp_path / "checks.i32", np.int32)
    assert checks[:3].tolist() == [0, 0, 0]
    plain = np.fromfile(tmp_path / "plain_rows.f32", np.float32).reshape(-1, 42)
    want = ctx.narf_descriptors(src.x, src.y, src.z, np.array([640 * 240 + 320, 640 * 200 + 300, -1], np.int32),
                                narf_desc_params(0.2, False))
    assert 1 <= len(want.desc) == checks[3] and np.array_equal(plain[:, 6:].view(np.uint32), want.desc.view(np.uint32))
