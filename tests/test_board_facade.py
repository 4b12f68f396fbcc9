"""BOARDLocalReferenceFrameEstimation of the C++ facade (include/pfx_pcl.hpp):
tests/cpp/board_facade_driver.cpp makes the calls of the reference's DESC_BOARD branch
(evaluation.cpp:372-393) through the generic wrapper (features.h:175-196) against it.  CPU: the
driver compiles and links against libpfx.so.  GPU: its rows equal Context.board_lrf bit for bit, the
wrapper's cast computes normals, is_dense is false exactly when a row holds a NaN,
findCorrespondences on ReferenceFrame (its x axis: dim 3 of stride 9) equals the C-ABI matcher, the
setters round-trip, and setFindHoles(true), a k-search and missing normals make compute() fail
loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "board_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("board_facade") / "board_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_board_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


def test_facade_declares_the_class_and_the_layout():
    hpp = open(os.path.join(ROOT, "include", "pfx_pcl.hpp")).read()
    assert "class BOARDLocalReferenceFrameEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT>" in hpp
    assert "DescriptorLayout<ReferenceFrame> { static constexpr int dim = 3, stride = 9; }" in hpp
    for setter in ("setTangentRadius", "setFindHoles", "setMarginThresh", "setCheckMarginArraySize",
                   "setHoleSizeProbThresh", "setSteepThresh"):
        assert setter in hpp and setter.replace("set", "get", 1) in hpp


@pytest.mark.gpu
def test_board_facade_matches_c_abi(ctx, driver, tmp_path):
    from parity import bits_equal
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    load = lambda name, w: np.fromfile(tmp_path / name, np.float32).reshape(-1, w)  # noqa: E731
    rows = {}
    for tag, path, n in (("src", PCD, 49), ("tgt", PCD_T, 48)):
        c = read_pcd(path)
        xyz = (c.x, c.y, c.z)
        nrm = ctx.normals(*xyz, 0.05)[:3]
        kp = load(f"{tag}_kp_xyz.f32", 3)
        assert len(kp) == n
        q = tuple(kp[:, i].copy() for i in range(3))
        got = load(f"{tag}_rf.f32", 9)
        assert bits_equal(got, ctx.board_lrf(*xyz, *nrm, *q, 0.08))
        assert np.isfinite(got[:48]).all(axis=1).sum() > 40
        rows[tag] = got
        if tag == "src":
            assert bits_equal(load("src_rf_tangent.f32", 9), ctx.board_lrf(*xyz, *nrm, *q, 0.08, tangent_radius=0.05))
    assert np.isnan(rows["src"][-1]).all()                           # the far keypoint: k = 0
    want_dense = [int(not np.isnan(a).any()) for a in (rows["src"], rows["tgt"])]
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == want_dense and want_dense[0] == 0
    # the wrapper's cast: BOARD is a FeatureFromNormals
    assert np.fromfile(tmp_path / "casts.i32", np.int32).tolist() == [1]
    # DescriptorLayout<ReferenceFrame>: the x axis alone, dim 3 of stride 9 (a NaN row matches nobody)
    corr = np.fromfile(tmp_path / "corr.i32", np.int32).reshape(-1, 2)
    q, m = ctx.correspondences(rows["src"][:, :3], rows["tgt"][:, :3])
    assert len(q) > 0 and np.array_equal(corr[:, 0], q) and np.array_equal(corr[:, 1], m)
    # the getters of a default object, then after every setter
    f32 = np.float32
    assert np.fromfile(tmp_path / "setters.f32", np.float32).tolist() == [
        0.0, 0.0, f32(0.85), 24.0, f32(0.2), f32(0.1), f32(0.03), 1.0, 0.5, 36.0, f32(0.3), 0.25]
    # find_holes, a k-search, no normals: PCL_ERROR and an empty output; the object works afterwards
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 0, 49, 49]
    assert "find_holes" in r.stderr
    assert ("[pcl::BOARDLocalReferenceFrameEstimation::computeFeature] Error! Search method set to k-neighborhood. "
            "Call setKSearch(0) and setRadiusSearch( radius ) to use this class.") in r.stderr
    assert r.stderr.count("[pcl::BOARDLocalReferenceFrameEstimation::compute]") >= 2
