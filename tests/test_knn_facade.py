"""The k-search half of the C++ facade (include/pfx_pcl.hpp): tests/cpp/knn_facade_driver.cpp runs
NormalEstimationOMP with setKSearch(10), PCL's "both radius and K" rule, BoundaryEstimation with
setKSearch(10) and KdTreeFLANN<PointXYZRGB>::nearestKSearch(p, 5) on the first 4,000 points of
tests/golden/clouds/indoor_source.pcd.  CPU: the driver compiles and links against libpfx.so.  GPU: its
normals equal Context.normals_knn bit for bit, its rows those of Context.knn_search, and the refusals
print their sentences and leave empty clouds."""
import os
import subprocess

import numpy as np
import pytest

from pcl_feature_extraction_amd import _native as NAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "knn_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
N = 4000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knn_facade") / "knn_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_knn_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


def test_facade_opt_in_is_the_normals_alone():
    hpp = open(os.path.join(ROOT, "include", "pfx_pcl.hpp")).read()
    assert hpp.count("this->accepts_k_search_ = true;") == 1
    ne = hpp[hpp.index("class NormalEstimationOMP"):hpp.index("class FPFHEstimation")]
    assert "this->accepts_k_search_ = true;" in ne and "pfx_normals_knn(" in ne
    assert "Both radius (%f) and K (%d) defined! Set one of them to zero first and then" in hpp
    assert "pfx_knn_search(" in hpp[hpp.index("class KdTreeFLANN<PointXYZRGB>"):]


@pytest.mark.gpu
def test_knn_facade_matches_the_python_calls(ctx, driver, tmp_path):
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    c = read_pcd(PCD)
    x, y, z = c.x[:N], c.y[:N], c.z[:N]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    got = np.fromfile(tmp_path / "normals.f32", np.float32).reshape(N, 4)
    want = ctx.normals_knn(x, y, z, 10)
    for col in range(4):
        assert np.array_equal(bits(got[:, col]), bits(want[col]))
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == [int(not np.isnan(want[0]).any())]
    # both set, neither set, a class without the path: empty outputs; then the object works again
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 0, N]
    assert ("[pcl::NormalEstimationOMP::compute] Both radius (0.050000) and K (10) defined! Set one of them to zero "
            "first and then re-run compute ().") in r.stderr
    assert "[pcl::NormalEstimationOMP::compute] initCompute failed" in r.stderr
    assert ("[pcl::BoundaryEstimation::compute] initCompute failed (needs an input cloud and a radius; k-NN search is "
            "not on the accelerated path)") in r.stderr
    q = np.arange(0, N, 250)
    counts, idx, d2 = ctx.knn_search(x, y, z, x[q] + np.float32(0.001), y[q], z[q], 5)
    assert np.fromfile(tmp_path / "knn_ret.i32", np.int32).tolist() == counts.tolist() == [5] * len(q)
    assert np.array_equal(np.fromfile(tmp_path / "knn_idx.i32", np.int32).reshape(-1, 5), idx)
    assert np.array_equal(bits(np.fromfile(tmp_path / "knn_d2.f32", np.float32).reshape(-1, 5)), bits(d2))
    nfin = int((np.isfinite(x) & np.isfinite(y) & np.isfinite(z)).sum())
    full = min(NAT.KNN_MAX_K, nfin)
    assert np.fromfile(tmp_path / "knn_edge.i32", np.int32).tolist() == [0, 0, 0, full, full]
    assert r.stderr.count("[pcl::KdTreeFLANN::nearestKSearch] k must be in [1, 256]") == 2
