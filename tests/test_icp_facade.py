"""IterativeClosestPoint and transformPointCloud of the C++ facade (include/pfx_pcl.hpp):
tests/cpp/icp_facade_driver.cpp makes the reference's setter and align sequence
(evaluation.cpp:863-885, :257) through it.  CPU: the driver compiles and links against libpfx.so.
GPU: transformation, fitness score, convergence and the aligned cloud equal Context.icp on the same
inputs by raw bits, and transformPointCloud equals the restatement's affine form."""
import os
import subprocess

import numpy as np
import pytest

import icp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "icp_facade_driver.cpp")
PCD = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd")
PCD_T = os.path.join(ROOT, "tests", "golden", "clouds", "indoor_target.pcd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_facade") / "icp_facade_driver")
    lib = os.path.join(ROOT, "pcl_feature_extraction_amd")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), SRC,
           "-L", lib, "-lpfx", f"-Wl,-rpath,{lib}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_icp_facade_compiles_and_links(driver):
    assert os.access(driver, os.X_OK)


@pytest.mark.gpu
def test_icp_facade_matches_c_abi(ctx, driver, tmp_path):
    from parity import bits_equal
    from pcl_feature_extraction_amd import icp_params
    r = subprocess.run([driver, PCD, PCD_T, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ref = R.build(tmp_path)
    src = np.fromfile(tmp_path / "src_xyz.f32", np.float32).reshape(-1, 3)
    tgt = np.fromfile(tmp_path / "tgt_xyz.f32", np.float32).reshape(-1, 3)
    assert len(src) > 2000 and len(tgt) > 2000
    s = tuple(np.ascontiguousarray(src[:, i]) for i in range(3))
    t = tuple(np.ascontiguousarray(tgt[:, i]) for i in range(3))
    guess = np.fromfile(tmp_path / "guess.f32", np.float32).reshape(4, 4)
    seen = []
    for prefix, g in (("", None), ("guess_", guess)):
        want = ctx.icp(*s, *t, icp_params(**R.REFERENCE), g)
        tf = np.fromfile(tmp_path / f"{prefix}tf.f32", np.float32).reshape(4, 4)
        score = np.fromfile(tmp_path / f"{prefix}score.f64", np.float64)
        flags = np.fromfile(tmp_path / f"{prefix}flags.i32", np.int32)
        aligned = np.fromfile(tmp_path / f"{prefix}aligned_xyz.f32", np.float32).reshape(-1, 3)
        moved = np.fromfile(tmp_path / f"{prefix}moved_xyz.f32", np.float32).reshape(-1, 3)
        rgb = np.fromfile(tmp_path / f"{prefix}rgb.u32", np.uint32).reshape(3, -1)
        assert bits_equal(tf, want.transformation)
        assert score.view(np.uint64)[0] == np.float64(want.fitness).view(np.uint64)
        assert flags.tolist() == [int(want.converged), want.state] and want.iterations > 2
        assert bits_equal(aligned, np.stack(want.aligned, 1))
        assert bits_equal(moved, np.stack(R.transform(ref, s, tf), 1))
        # the aligned and the moved cloud keep the source's other fields
        assert np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[0], rgb[2]) and len(np.unique(rgb[0])) > 100
        seen.append(tf)
    assert not bits_equal(seen[0], seen[1])  # the guess was used
