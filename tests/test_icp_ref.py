"""Analytic cases that pin tests/cpp/icp_ref.cpp, the CPU restatement the GPU ICP is compared
with bit for bit (test_gpu_icp.py).  Parity of the restatement with real PCL is unpinned."""
import numpy as np
import pytest

import icp_cases as C
import icp_ref as R


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("icp_ref"))


def run(lib, case):
    s, t, p, g = case
    return R.icp(lib, s, t, p, g)


IDENTITY = np.eye(4, dtype=np.float32)


def test_identical_clouds_converge_in_one_iteration(lib):
    r = run(lib, C.identical())
    assert r.iterations == 1 and r.state == R.TRANSFORM and r.converged
    assert len(r.first_d2) == 343 and not r.first_d2.any()
    assert np.array_equal(r.first_src, r.first_tgt)
    assert np.abs(r.transformation - IDENTITY).max() <= 2 * 343 * 2.0 ** -24 * 0.7


def test_shifted_lattice_takes_two_iterations(lib):
    s, t, p, g = C.shifted_lattice()
    r = R.icp(lib, s, t, p, g)
    n = len(s[0])
    assert n == 512 and r.n_last == n
    assert r.iterations == 2 and r.state == R.TRANSFORM and r.converged
    # worst case of a recursive float sum of n terms: n 2^-24 max|coord| per mean, two means
    bound = 2 * n * 2.0 ** -24 * max(np.abs(v).max() for v in s + t)
    assert np.abs(r.transformation[:3, 3].astype(np.float64) - C.DELTA).max() <= bound
    assert np.array_equal(r.first_src, r.first_tgt)  # every point found its own partner
    assert r.fitness < 1e-9


def test_beyond_the_cap_there_are_no_correspondences(lib):
    r = run(lib, C.far_apart())
    assert r.state == R.NO_CORRESPONDENCES and not r.converged and r.iterations == 0 and r.n_last == 0
    assert np.array_equal(r.transformation, IDENTITY)
    assert 80.0 < r.fitness < 100.0  # the fitness score has no cap


def test_iteration_cap(lib):
    r = run(lib, C.one_iteration())
    assert r.iterations == 1 and r.state == R.ITERATIONS and r.converged


def test_lowest_target_index_wins_a_tie(lib):
    r = run(lib, C.ties())
    assert list(r.first_src) == list(range(7))
    assert list(r.first_tgt) == [0, 2, 4, 6, 8, 10, 12]
    assert np.array_equal(r.first_d2[:6], np.full(6, 0.03125 ** 2, np.float32))


def test_cap_is_inclusive_at_equality(lib):
    r = run(lib, C.exact_cap())
    assert list(r.first_src) == [0, 2, 3, 4, 5] and list(r.first_tgt) == [0, 2, 3, 4, 5]
    assert r.first_d2[0] == np.float32(0.25) and r.n_last == 5


def test_non_finite_points_are_skipped(lib):
    dirty, clean = C.with_nans()
    a, b = run(lib, dirty), run(lib, clean)
    # 4 source points are gone, and the partners of the 3 missing target points find nothing within the cap
    assert a.n_last == b.n_last == 512 - 4 - 3
    assert np.array_equal(a.transformation.view(np.uint32), b.transformation.view(np.uint32))
    assert a.fitness == b.fitness and (a.iterations, a.state) == (b.iterations, b.state) == (2, R.TRANSFORM)


def test_depth_blocks_change_the_sum_only_past_one_block(lib):
    """Up to PFX_ICP_GEMM_DEPTH pairs sigma is one sequential chain; the list_length clouds straddle
    that edge, and the restatement must at least run them to the same kind of result."""
    for n in (1023, 1024, 1025, 2049):
        r = run(lib, C.list_length(n))
        assert r.n_last == n and r.converged and r.state == R.TRANSFORM
        assert np.abs(r.transformation[:3, 3].astype(np.float64) - 0.5 * C.DELTA).max() <= 2 * n * 2.0 ** -24 * 1.3


def test_two_pairs_are_too_few(lib):
    r = run(lib, C.list_length(2))
    assert r.state == R.NO_CORRESPONDENCES and r.n_last == 2 and r.iterations == 0


def test_transform_is_the_affine_form(lib):
    T = np.array([[0.5, 0.25, -1, 3], [2, 1, 0.125, -4], [1, -2, 4, 0.5], [0, 0, 0, 1]], np.float32)
    x, y, z = (np.array([1, 3, -2], np.float32), np.array([2, 0.5, 8], np.float32), np.array([4, -1, 0.25], np.float32))
    ox, oy, oz = R.transform(lib, (x, y, z), T)
    assert list(ox) == [0.5 + 0.5 - 4 + 3, 1.5 + 0.125 + 1 + 3, -1 + 2 - 0.25 + 3]
    assert list(oy) == [2 + 2 + 0.5 - 4, 6 + 0.5 - 0.125 - 4, -4 + 8 + 0.03125 - 4]
    assert list(oz) == [1 - 4 + 16 + 0.5, 3 - 1 - 4 + 0.5, -2 - 16 + 1 + 0.5]
