"""IntensitySpinEstimation of the C++ facade (include/pfx_pcl.hpp):
tests/cpp/intensity_spin_facade_driver.cpp makes the calls of the reference's DESC_INT_SPIN branch
(evaluation.cpp:466-514) against it.  CPU: the driver compiles and links against libpfx.so.  GPU: its
rows equal Context.intensity_spin bit for bit under PCL 1.7's indexing rule (row i describes the
*surface's* i-th point), is_dense follows the NaN rows, findCorrespondences on Histogram<20> equals
the C-ABI matcher, and what PCL would read or write out of bounds fails loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "intensity_spin_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("intensity_spin_facade") / "intensity_spin_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_intensity_spin_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
def test_intensity_spin_facade_matches_c_abi(ctx, driver, tmp_path):
    from parity import bits_equal
    from pcl_feature_extraction_amd import rgb_to_intensity
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = {}
    for tag, path in (("src", PCD), ("tgt", PCD_T)):
        c = read_pcd(path)
        xyz = (c.x, c.y, c.z)
        inten = rgb_to_intensity(np.ascontiguousarray(c.fields["rgb"]).view(np.uint32))
        n = len(np.fromfile(tmp_path / f"{tag}_kp_xyz.f32", np.float32).reshape(-1, 3))
        assert n == 24
        # row i describes *surface* point i, whatever the keypoints are
        want = ctx.intensity_spin(*xyz, inten, *(v[:n] for v in xyz), 0.08)
        got = np.fromfile(tmp_path / f"{tag}_ispin.f32", np.float32).reshape(-1, 20)
        assert bits_equal(got, want)
        rows[tag] = got
    want_dense = [int(not np.isnan(rows[t]).any()) for t in ("src", "tgt")]
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == want_dense
    assert want_dense == [1, 1]   # every cloud point is its own neighbour
    corr = np.fromfile(tmp_path / "corr_ispin.i32", np.int32).reshape(-1, 2)
    q, m = ctx.correspondences(rows["src"], rows["tgt"])
    assert np.array_equal(corr[:, 0], q) and np.array_equal(corr[:, 1], m)
    # an index beyond the surface and 4 x 4 bins into Histogram<20>: PCL_ERROR and an empty output; the
    # object works afterwards; the defaults are PCL's
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 24, 4, 5, 1]
    assert r.stderr.count("[pcl::IntensitySpinEstimation::compute]") >= 2
