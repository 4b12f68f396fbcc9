"""BoundaryEstimation of the C++ facade (include/pfx_pcl.hpp): tests/cpp/boundary_facade_driver.cpp
makes the calls of the reference's DESC_BOUNDARY branch (evaluation.cpp:394-415) up to compute through
the generic wrapper (features.h:175-196) against it.  CPU: the driver compiles and links against
libpfx.so.  GPU: its bytes equal Context.boundary called with the FIRST nq normals of the surface as
the queries' normals (PCL's indexing, which this test pins: the keypoints' own normals give other
flags), the wrapper's cast computes normals, a row without a neighbour is 0 and clears is_dense, the
setter round-trips, and a k-search, missing normals, more input points than normals and a threshold
below pi / 64 make compute() fail loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "boundary_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("boundary_facade") / "boundary_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_boundary_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


def test_facade_declares_the_class():
    hpp = open(os.path.join(ROOT, "include", "pfx_pcl.hpp")).read()
    assert "class BoundaryEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT>" in hpp
    assert "struct Boundary { uint8_t boundary_point = 0; };" in hpp
    assert "setAngleThreshold" in hpp and "getAngleThreshold" in hpp
    assert "static_cast<float>(M_PI) / 2.0f" in hpp                  # PCL's default
    assert "DescriptorLayout<Boundary>" not in hpp                   # no KdTreeFLANN<Boundary>


@pytest.mark.gpu
def test_boundary_facade_matches_c_abi(ctx, driver, tmp_path):
    from pcl_feature_extraction_amd.pcd import read_pcd
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = {}
    for tag, path, n in (("src", PCD, 49), ("tgt", PCD_T, 48)):
        c = read_pcd(path)
        xyz = (c.x, c.y, c.z)
        nrm = ctx.normals(*xyz, 0.05)[:3]
        kp = np.fromfile(tmp_path / f"{tag}_kp_xyz.f32", np.float32).reshape(-1, 3)
        assert len(kp) == n
        q = tuple(kp[:, i].copy() for i in range(3))
        first = tuple(v[:n] for v in nrm)                            # normals [0, nq): PCL's indexing
        got = np.fromfile(tmp_path / f"{tag}_flags.u8", np.uint8)
        want = ctx.boundary(*xyz, *q, *first, 0.08)
        assert np.array_equal(got, np.where(want == 255, 0, want).astype(np.uint8)), tag
        assert set(got.tolist()) == {0, 1}
        rows[tag] = want
        if tag == "src":
            wide = ctx.boundary(*xyz, *q, *first, 0.08, 2.5)
            assert np.array_equal(np.fromfile(tmp_path / "src_flags_wide.u8", np.uint8), np.where(wide == 255, 0, wide))
            assert wide.sum() < want.sum()
            # the quirk decides rows: the keypoints' own normals (every (n / 48)-th of the cloud's) flag others
            step = len(c.x) // 48
            own_rows = [i for i in range(0, len(c.x), step) if np.isfinite([c.x[i], c.y[i], c.z[i]]).all()][:48]
            assert np.array_equal(np.stack([v[own_rows] for v in xyz], 1), kp[:48])
            own = ctx.boundary(*xyz, *(v[:48] for v in q), *(v[own_rows] for v in nrm), 0.08)
            assert (own != want[:48]).any()
    assert rows["src"][-1] == 255 and (rows["src"][:-1] != 255).all()     # the far keypoint: k = 0
    assert np.fromfile(tmp_path / "dense.i32", np.int32).tolist() == [0, 1]
    # the wrapper's cast: BoundaryEstimation is a FeatureFromNormals
    assert np.fromfile(tmp_path / "casts.i32", np.int32).tolist() == [1]
    f32 = np.float32
    assert np.fromfile(tmp_path / "setters.f32", np.float32).tolist() == [f32(np.pi) / f32(2), 2.5]
    # a k-search, no normals, more input points than normals, a threshold below pi / 64: PCL_ERROR and
    # an empty output; the object works afterwards
    assert np.fromfile(tmp_path / "checks.i32", np.int32).tolist() == [0, 0, 0, 0, 49]
    assert "pi / 64" in r.stderr and "beyond the search surface" in r.stderr
    assert r.stderr.count("[pcl::BoundaryEstimation::compute]") >= 4
