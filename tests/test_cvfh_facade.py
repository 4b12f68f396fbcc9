"""CVFHEstimation of the C++ facade (include/pfx_pcl.hpp): tests/cpp/cvfh_facade_driver.cpp makes the
calls of the reference's DESC_CVFH branch (evaluation.cpp:649-675) through the generic wrapper
(features.h:175-196) and the matching (features.h:224-273) against it.  CPU: the driver compiles and
links against libpfx.so.  GPU: its rows equal Context.cvfh on the FIRST K POINTS OF THE CLOUD (PCL's
indexing on this path, which this test pins), the second compute on the same object is correct, the
setKSearch rule holds, more keypoints than surface points fail loudly, and correspondences come out."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cvfh_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cvfh_facade") / "cvfh_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_cvfh_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


def test_facade_declares_the_class():
    hpp = open(os.path.join(ROOT, "include", "pfx_pcl.hpp")).read()
    assert "class CVFHEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT>" in hpp
    assert "struct VFHSignature308 { float histogram[308]; };" in hpp
    assert "DescriptorLayout<VFHSignature308>" in hpp
    for name in ("setViewPoint", "setRadiusNormals", "setClusterTolerance", "setEPSAngleThreshold",
                 "setCurvatureThreshold", "setMinPoints", "setNormalizeBins", "getCentroidClusters",
                 "getCentroidNormalClusters"):
        assert name in hpp, name


@pytest.mark.gpu
def test_cvfh_facade_matches_c_abi(ctx, driver, tmp_path):
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    counts = np.fromfile(tmp_path / "counts.i32", np.int32).tolist()
    assert counts[:2] == [1500, 1500]
    rows = {}
    for k, (tag, path) in enumerate((("src", PCD), ("tgt", PCD_T))):
        c = read_pcd(path)
        s = (c.x, c.y, c.z) + tuple(ctx.normals(c.x, c.y, c.z, 0.05))
        want = ctx.cvfh(*s, indices=np.arange(1500, dtype=np.int32))      # the first K points of the cloud
        got = np.fromfile(tmp_path / f"{tag}_rows.f32", np.float32).reshape(-1, 308)
        assert got.shape == want.rows.shape and np.array_equal(got.view(np.uint32), want.rows.view(np.uint32)), tag
        about = np.fromfile(tmp_path / f"{tag}_about.f32", np.float32).reshape(-1, 6)
        assert np.array_equal(about[:, :3].view(np.uint32), want.centroids.view(np.uint32))
        assert np.array_equal(about[:, 3:].view(np.uint32), want.dominant_normals.view(np.uint32))
        assert counts[2 + 2 * k: 4 + 2 * k] == [len(got), 1]             # width = rows, height = 1
        assert (got[:, 180:].sum(1) == 1500).all()                       # every indexed point in the viewpoint block
        rows[tag] = got
        print(tag, "rows", len(got))
    assert np.fromfile(tmp_path / "casts.i32", np.int32).tolist() == [1]
    # the matching: mutual nearest rows, recomputed here in float64
    d = ((rows["src"][:, None, :].astype(np.float64) - rows["tgt"][None, :, :]) ** 2).sum(2)
    s2t, t2s = d.argmin(1), d.argmin(0)
    pairs = [[i, int(j)] for i, j in enumerate(s2t) if t2s[j] == i]
    corr = np.fromfile(tmp_path / "corr.i32", np.int32).reshape(-1, 2).tolist()
    assert len(corr) >= 1 and corr == pairs
    # k = 1 from the constructor with a radius set: PCL_ERROR as initCompute; setKSearch(0) cures it; more
    # keypoints than surface points: refused; the object works afterwards
    n_src = len(rows["src"])
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, n_src, 0, n_src]
    assert "Both radius and K defined" in r.stderr and "an index is outside the surface" in r.stderr
