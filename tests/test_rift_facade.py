"""IntensityGradientEstimation / RIFTEstimation / IntensityGradient of the C++ facade
(include/pfx_pcl.hpp): tests/cpp/rift_facade_driver.cpp makes the calls of the reference's
DESC_INT_GRAD and DESC_RIFT branches (evaluation.cpp:419-462, 720-762; tools.h:40-54) against it.
CPU: the driver compiles and links against libpfx.so.  GPU: its rows equal Context.intensity_gradient
/ Context.rift bit for bit under PCL 1.7's indexing rules (the gradient's normal is the *cloud's*
i-th, RIFT's row i describes the *surface's* i-th point), is_dense follows the NaN rows,
findCorrespondences on both descriptor types equals the C-ABI matcher, and what PCL would read or
write out of bounds fails loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rift_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rift_facade") / "rift_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_rift_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
def test_rift_facade_matches_c_abi(ctx, driver, tmp_path):
    from parity import bits_equal
    from pcl_feature_extraction_amd import rgb_to_intensity
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    load = lambda name, w: np.fromfile(tmp_path / name, np.float32).reshape(-1, w)  # noqa: E731
    rows, dense = {}, []
    for tag, path, n in (("src", PCD, 49), ("tgt", PCD_T, 48)):
        c = read_pcd(path)
        xyz = (c.x, c.y, c.z)
        inten = rgb_to_intensity(np.ascontiguousarray(c.fields["rgb"]).view(np.uint32))
        nrm = ctx.normals(*xyz, 0.05)[:3]
        kp = load(f"{tag}_kp_xyz.f32", 3)
        assert len(kp) == n
        q = tuple(kp[:, i].copy() for i in range(3))
        # the gradient: the neighbours of keypoint i, the normal of *cloud* point i
        want_g = ctx.intensity_gradient(*xyz, inten, *q, *(v[:n] for v in nrm), 0.08)
        got_g = load(f"{tag}_igrad.f32", 3)
        assert bits_equal(got_g, want_g)
        # Tools::computeGradient: the whole cloud at the normal radius
        cloud_g = ctx.intensity_gradient(*xyz, inten, *xyz, *nrm, 0.05, same_as_surface=True)
        got_cg = load(f"{tag}_cloud_grad.f32", 3)
        assert bits_equal(got_cg, cloud_g)
        # RIFT: row i describes *surface* point i
        want_r = ctx.rift(*xyz, *(np.ascontiguousarray(cloud_g[:, i]) for i in range(3)), *(v[:n] for v in xyz), 0.08, 4, 8)
        got_r = load(f"{tag}_rift.f32", 32)
        assert bits_equal(got_r, want_r) and np.isfinite(got_r).all(axis=1).sum() > n // 2
        rows[tag] = (got_g, got_r)
        dense.append((got_g, got_r, got_cg))
    assert np.isnan(rows["src"][0][-1]).all()       # the far keypoint: k = 0, a NaN gradient row
    (sg, sr, scg), (tg, tr, tcg) = dense
    want_dense = [int(not np.isnan(a).any()) for a in (sg, tg, sr, tr, scg, tcg)]
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == want_dense and want_dense[0] == 0
    for name, which in (("corr_igrad.i32", 0), ("corr_rift.i32", 1)):
        corr = np.fromfile(tmp_path / name, np.int32).reshape(-1, 2)
        q, m = ctx.correspondences(rows["src"][which], rows["tgt"][which])
        assert len(q) > 0 and np.array_equal(corr[:, 0], q) and np.array_equal(corr[:, 1], m)
    # an index beyond the surface (gradient, RIFT), a gradient cloud of another size, 4 x 4 bins into
    # Histogram<32>: PCL_ERROR and an empty output; and the object works afterwards
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 0, 0, 49]
    assert "[pcl::IntensityGradientEstimation::compute]" in r.stderr
    assert r.stderr.count("[pcl::RIFTEstimation::compute]") >= 3
