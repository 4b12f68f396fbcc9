"""SpinImageEstimation / Histogram<153> of the C++ facade (include/pfx_pcl.hpp):
tests/cpp/spin_facade_driver.cpp writes the reference's DESC_SPIN_IMAGE branch
(evaluation.cpp:518-552) against it, the axes being the normals of the sparse keypoint cloud among
itself.  CPU: the driver compiles and links against libpfx.so.  GPU: its rows equal
Context.spin_image on the same inputs bit for bit, the rows of keypoints with NaN normals are
finite with mass in alpha_bin 0 only, findCorrespondences on PointCloud<Histogram<153>> equals the
C-ABI matcher, and what the accelerated path refuses fails loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "spin_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spin_facade") / "spin_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_spin_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
def test_spin_facade_matches_c_abi(ctx, driver, tmp_path):
    from parity import bits_equal
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = {}
    for tag, path, n in (("src", PCD, 65), ("tgt", PCD_T, 64)):
        c = read_pcd(path)
        kp = np.fromfile(tmp_path / f"{tag}_kp_xyz.f32", np.float32).reshape(-1, 3)
        kn = np.fromfile(tmp_path / f"{tag}_kp_normals.f32", np.float32).reshape(-1, 3)
        got = np.fromfile(tmp_path / f"{tag}_spin.f32", np.float32).reshape(-1, 153)
        q = tuple(kp[:, i].copy() for i in range(3))
        axes = ctx.normals(*q, 0.05)[:3]          # the keypoint cloud among itself
        assert len(kp) == n and bits_equal(kn, np.stack(axes, 1))
        want = ctx.spin_image(c.x, c.y, c.z, *q, *axes, 0.08)
        assert bits_equal(got, want)
        nan = np.isnan(kn[:, 0])
        assert 32 < nan.sum() < n - 8             # mostly NaN; the four clusters have normals
        img = got.reshape(-1, 9, 17)
        assert np.isfinite(img[nan]).all() and not img[nan][:, 1:].any()
        assert img[nan][:, 0].any(axis=1).sum() > 32 and img[~nan][:, 1:].any()
        rows[tag] = got
    assert not rows["src"][-1].any()              # the far keypoint: k = 0, a zero row
    corr = np.fromfile(tmp_path / "corr.i32", np.int32).reshape(-1, 2)
    q, m = ctx.correspondences(rows["src"], rows["tgt"])
    assert len(q) > 0 and np.array_equal(corr[:, 0], q) and np.array_equal(corr[:, 1], m)
    # radial, angular, custom axis, mismatched normals, wrong width: PCL_ERROR and an empty output;
    # too few neighbours: pcl::PCLException, and the object works afterwards
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 0, 0, 0, 1]
    assert r.stderr.count("[pcl::SpinImageEstimation::compute]") >= 6 and "too few neighbours" in r.stderr
