"""SHOTColorEstimationOMP / SHOT1344 of the C++ facade (include/pfx_pcl.hpp):
tests/cpp/shot_color_facade_driver.cpp writes the reference's DESC_SHOT_COLOR branch
(evaluation.cpp:786-805) against it.  CPU: the driver compiles and links against libpfx.so.  GPU:
its rows equal Context.shot_color on the same inputs bit for bit, is_dense follows the NaN row, and
findCorrespondences on PointCloud<SHOT1344> equals the C-ABI matcher."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shot_color_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shot_color_facade") / "shot_color_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_shot_color_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
def test_shot_color_facade_matches_c_abi(ctx, driver, tmp_path):
    from parity import bits_equal
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = {}
    for tag, path in (("src", PCD), ("tgt", PCD_T)):
        c = read_pcd(path)
        rgb = np.ascontiguousarray(c.fields["rgb"]).view(np.uint32)
        nrm = ctx.normals(c.x, c.y, c.z, 0.05)[:3]
        kp = np.fromfile(tmp_path / f"{tag}_kp_xyz.f32", np.float32).reshape(-1, 3)
        kp_rgb = np.fromfile(tmp_path / f"{tag}_kp_rgb.u32", np.uint32)
        got = np.fromfile(tmp_path / f"{tag}_shot.f32", np.float32).reshape(-1, 1353)
        desc, rf = ctx.shot_color(c.x, c.y, c.z, *nrm, rgb, kp[:, 0].copy(), kp[:, 1].copy(), kp[:, 2].copy(),
                                  kp_rgb, 0.08)
        assert len(kp) >= 64 and len(kp_rgb) == len(kp)
        assert bits_equal(got[:, :1344], desc) and bits_equal(got[:, 1344:], rf)
        rows[tag] = np.ascontiguousarray(got[:, :1344])
    # the source's last keypoint lies far from the cloud: a NaN row, so is_dense is false there only
    assert np.isnan(rows["src"][-1]).all() and not np.isnan(rows["src"][:-1]).any()
    tgt_dense = int(not np.isnan(rows["tgt"]).any())
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == [0, tgt_dense]
    corr = np.fromfile(tmp_path / "corr.i32", np.int32).reshape(-1, 2)
    q, m = ctx.correspondences(rows["src"], rows["tgt"])
    assert len(q) > 0 and np.array_equal(corr[:, 0], q) and np.array_equal(corr[:, 1], m)
