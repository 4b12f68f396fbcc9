"""The CPU restatements of the moment invariants and the principal curvatures
(tests/cpp/moments_ref.cpp) pinned by contract, not by themselves: closed-form rows with exact
answers, the special rows of pfx.h, the proof that the neighbour order decides bits (so the GPU
comparison of tests/test_gpu_moments.py has teeth) and that the (root2 * scale) / scale detour of
computeCorrespondingEigenVector is exercised."""
import numpy as np
import pytest

import moments_cases as K
import moments_ref as P
from parity import bits

FAR = (9.0e3, 9.0e3, 9.0e3)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("moments_ref"))


def all_nan(row):
    return (bits(row) == K.NAN_BITS).all()


def exact(row, want):
    return np.array_equal(bits(np.asarray(row, np.float32)), bits(np.float32(want)))


# ---- moment invariants ----

@pytest.mark.parametrize("abc", [(2.0 ** -6, 2.0 ** -7, 2.0 ** -5), (2.0 ** -6, 2.0 ** -6, 2.0 ** -6),
                                 (2.0 ** -5, 2.0 ** -8, 2.0 ** -7)])
def test_axis_points_give_the_closed_form_exactly(ref, abc):
    xyz, want = K.axis_case(*abc)
    got = P.moments(ref, *xyz, *K.points(K.Q0), K.R)
    assert (got.neighbors, got.kmax) == (7, 7)
    assert all(np.float64(np.float32(w)) == w for w in want)      # the answers are float32 numbers
    assert exact(got.out[0], want), (got.out[0], want)
    # the walk's direction does not matter where every sum is exact
    assert exact(P.moments(ref, *xyz, *K.points(K.Q0), K.R, reversed_order=True).out[0], want)


def test_diagonal_pair_has_rank_one(ref):
    xyz, want = K.diagonal_case()
    got = P.moments(ref, *xyz, *K.points(K.Q0), K.R)
    assert got.kmax == 2 and exact(got.out[0], want) and want[0] > 0


def test_moments_special_rows(ref):
    one = K.points(K.Q0)
    q = K.points(K.Q0, FAR, (np.nan, 2.0, 3.0), (1.0, np.inf, 3.0))
    got = P.moments(ref, *one, *q, K.R)
    assert exact(got.out[0], (0.0, 0.0, 0.0))                      # k = 1: +0 +0 +0
    assert all_nan(got.out[1:]) and (got.neighbors, got.kmax) == (1, 1)
    # duplicates of one point: k = 4, every t is 0
    got = P.moments(ref, *K.points(K.Q0, K.Q0, K.Q0, K.Q0), *one, K.R)
    assert got.kmax == 4 and exact(got.out[0], (0.0, 0.0, 0.0))
    # no surface at all
    none = tuple(v[:0] for v in one)
    got = P.moments(ref, *none, *one, K.R)
    assert all_nan(got.out) and got.neighbors == 0
    # a non-finite surface point is no neighbour
    xyz, want = K.axis_case()
    x = np.append(xyz[0], np.float32(np.nan))
    got = P.moments(ref, x, np.append(xyz[1], np.float32(2.0)), np.append(xyz[2], np.float32(3.0)), *one, K.R)
    assert got.kmax == 7 and exact(got.out[0], want)


def test_moments_agree_with_float64_on_blobs(ref):
    """Sequential float32 sums of k = 300 terms of size s carry about k eps s of error: 1e-4
    relative to each invariant's own scale (j1 ~ k side^2 / 4) is a dozen times that."""
    c = K.order_case(k=300, blobs=3)
    got = P.moments(ref, *c["xyz"], *c["q"], K.R)
    p = np.stack(c["xyz"], 1).astype(np.float64)
    for row, lo in zip(got.out, c["rows"]):
        t = p[lo:lo + 300] - p[lo:lo + 300].mean(axis=0)
        m = t.T @ t
        j1 = np.trace(m)
        j2 = m[0, 0] * m[1, 1] + m[0, 0] * m[2, 2] + m[1, 1] * m[2, 2] - m[0, 1] ** 2 - m[0, 2] ** 2 - m[1, 2] ** 2
        j3 = np.linalg.det(m)
        assert abs(row[0] - j1) < 1e-4 * j1 and abs(row[1] - j2) < 1e-4 * j1 ** 2 and abs(row[2] - j3) < 1e-4 * j1 ** 3


# ---- principal curvatures ----

def test_equal_normals_give_zero_curvatures_and_a_nan_direction(ref):
    xyz = K.ring(8)
    for n in (K.Z, (0.5, 0.25, 1.0)):      # (sums of eight stay exact)
        got = P.curvatures(ref, *xyz, *K.vectors(8, n), *K.points(K.Q0), *K.vectors(1, K.Z), K.R)
        assert got.kmax == 8 and all_nan(got.out[0, :3]) and exact(got.out[0, 3:], (0.0, 0.0))
    # k = 1 is the same case
    got = P.curvatures(ref, *K.points(K.Q0), *K.vectors(1, (0.5, 0.25, 1.0)), *K.points(K.Q0), *K.vectors(1, K.Z), K.R)
    assert got.kmax == 1 and all_nan(got.out[0, :3]) and exact(got.out[0, 3:], (0.0, 0.0))


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_known_spread(ref, m):
    xyz, nrm, want = K.spread_case(m)
    got = P.curvatures(ref, *xyz, *nrm, *K.points(K.Q0), *K.vectors(1, K.Z), K.R)
    assert got.kmax == 8 and exact(got.out[0], want), (got.out[0], want)


def test_curvature_special_rows(ref):
    xyz, nrm, want = K.spread_case(2)
    q = K.points(K.Q0, FAR, (np.nan, 2.0, 3.0), K.Q0)
    qn = K.f32([0.0, 0.0, 0.0, np.nan], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0])
    got = P.curvatures(ref, *xyz, *nrm, *q, *qn, K.R)
    assert exact(got.out[0], want) and all_nan(got.out[1:3]) and (got.neighbors, got.kmax) == (16, 8)
    assert all_nan(got.out[3])                                     # a NaN query normal: every projection is NaN
    n = tuple(v.copy() for v in nrm)
    n[1][3] = np.nan                                               # a NaN normal among the neighbours
    got = P.curvatures(ref, *xyz, *n, *K.points(K.Q0), *K.vectors(1, K.Z), K.R)
    assert got.kmax == 8 and all_nan(got.out[0])


def test_curvatures_agree_with_float64_on_blobs(ref):
    """pc1 and pc2 are the two largest eigenvalues of the projected normals' covariance over k; the
    direction is the largest's eigenvector up to sign.  computeRoots is a closed form in float32:
    1e-4 of the largest eigenvalue (about 1/3 here) is some hundreds of float epsilons."""
    c = K.order_case(k=300, blobs=3)
    got = P.curvatures(ref, *c["xyz"], *c["normals"], *c["q"], *c["qnormals"], K.R)
    nr = np.stack(c["normals"], 1).astype(np.float64)
    for row, lo, n in zip(got.out, c["rows"], np.stack(c["qnormals"], 1).astype(np.float64)):
        pr = nr[lo:lo + 300] @ (np.eye(3) - np.outer(n, n)).T
        d = pr - pr.mean(axis=0)
        w, v = np.linalg.eigh(d.T @ d)
        assert abs(row[3] - w[2] / 300) < 1e-4 * w[2] / 300 and abs(row[4] - w[1] / 300) < 1e-4 * w[2] / 300
        assert abs(abs(np.dot(row[:3], v[:, 2])) - 1.0) < 1e-4


# ---- the order and the detour ----

def test_the_neighbour_order_decides_bits(ref):
    c = K.order_case()
    a = P.moments(ref, *c["xyz"], *c["q"], K.R)
    b = P.moments(ref, *c["xyz"], *c["q"], K.R, reversed_order=True)
    assert a.kmax == c["k"] and (bits(a.out) != bits(b.out)).any(axis=1).sum() >= len(a.out) // 2
    assert np.abs(a.out - b.out).max() <= 1e-4 * np.abs(a.out).max()
    a = P.curvatures(ref, *c["xyz"], *c["normals"], *c["q"], *c["qnormals"], K.R)
    b = P.curvatures(ref, *c["xyz"], *c["normals"], *c["q"], *c["qnormals"], K.R, reversed_order=True)
    assert (bits(a.out) != bits(b.out)).any(axis=1).sum() >= len(a.out) // 2
    assert np.abs(a.out - b.out).max() <= 1e-4


def test_the_eigenvalue_detour_is_exercised(ref):
    """computeCorrespondingEigenVector subtracts (root2 * scale) / scale, not root2: on some rows the
    two differ in bits, so a kernel that passes the root straight on cannot match."""
    c = K.smooth_blobs()
    got = P.curvatures(ref, *c["xyz"], *c["normals"], *c["xyz"], *c["normals"], K.R)
    print("detour rows:", got.detours, "of", len(got.out))
    assert got.detours >= 1 and np.isfinite(got.out).all()
