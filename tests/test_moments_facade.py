"""MomentInvariantsEstimation / PrincipalCurvaturesEstimation and their point types of the C++ facade
(include/pfx_pcl.hpp): tests/cpp/moments_facade_driver.cpp makes the calls of the reference's
DESC_MOMENT_INV and DESC_PPAL_CURV branches (evaluation.cpp:554-572, 696-715) through one generic
wrapper (features.h:175-196) against it.  CPU: the driver compiles and links against libpfx.so.
GPU: its rows equal Context.moment_invariants / Context.principal_curvatures bit for bit under PCL
1.7's indexing rule (the curvatures' query normal is the *cloud's* i-th), the wrapper's cast computes
normals for the curvatures alone, is_dense follows the NaN values, findCorrespondences on both
descriptor types equals the C-ABI matcher, and what PCL would read out of bounds fails loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "moments_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("moments_facade") / "moments_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_moments_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
def test_moments_facade_matches_c_abi(ctx, driver, tmp_path):
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
        got_m, got_p = load(f"{tag}_mi.f32", 3), load(f"{tag}_pc.f32", 5)
        assert bits_equal(got_m, ctx.moment_invariants(*xyz, *q, 0.08))
        # the curvatures: the neighbours of keypoint i, the query normal of *cloud* point i
        assert bits_equal(got_p, ctx.principal_curvatures(*xyz, *nrm, *q, *(v[:n] for v in nrm), 0.08))
        assert np.isfinite(got_m[:48]).all() and np.isfinite(got_p[:48]).all(axis=1).sum() > 24
        rows[tag] = (got_m, got_p)
    assert np.isnan(rows["src"][0][-1]).all() and np.isnan(rows["src"][1][-1]).all()   # the far keypoint: k = 0
    want_dense = [int(not np.isnan(a).any()) for a in (rows["src"][0], rows["tgt"][0], rows["src"][1], rows["tgt"][1])]
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == want_dense and want_dense[0] == want_dense[2] == 0
    assert want_dense[1] == 1
    # the wrapper's cast: no normals for the moment invariants, normals for the curvatures
    assert np.fromfile(tmp_path / "casts.i32", np.int32).tolist() == [0, 1]
    # DescriptorLayout: dim 3 of stride 3, and dim 3 (the principal direction alone) of stride 5
    for name, which in (("corr_mi.i32", 0), ("corr_pc.i32", 1)):
        corr = np.fromfile(tmp_path / name, np.int32).reshape(-1, 2)
        q, m = ctx.correspondences(rows["src"][which][:, :3], rows["tgt"][which][:, :3])
        assert len(q) > 0 and np.array_equal(corr[:, 0], q) and np.array_equal(corr[:, 1], m)
    # more keypoints than normals, no normals, normals of another size, no input: PCL_ERROR and an empty
    # output; and the objects work afterwards
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 0, 0, 49, 49]
    assert r.stderr.count("[pcl::PrincipalCurvaturesEstimation::compute]") >= 3
    assert "[pcl::MomentInvariantsEstimation::compute]" in r.stderr
