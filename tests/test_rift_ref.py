"""The CPU restatements of the intensity gradient and of RIFT (tests/cpp/rift_ref.cpp) pinned by
contract, not by themselves: closed-form rows, the special rows of pfx.h, Eigen 3.2's float summation
order against a direct Python statement of it, and the proof that the neighbour order decides bits
(so the GPU comparison of tests/test_gpu_rift.py has teeth)."""
import numpy as np
import pytest

import rift_cases as K
import rift_ref as P
from parity import bits

Z = (0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("rift_ref"))


def all_nan(row):
    return (bits(row) == K.NAN_BITS).all()


def columns(row, D=4, G=8):
    """row[gi * D + di] -> (G, D)."""
    return np.asarray(row).reshape(G, D)


# ---- the intensity gradient ----

def test_gradient_of_a_linear_intensity_on_a_plane(ref):
    """A = diag(s, s, 0) exactly and b = (a s, b s, 0) exactly (rift_cases.plane_case): the system has
    condition number 1 on its rank-two part, so the only error is the Householder QR's own, a few
    tens of float epsilons relative to |x| = 2.1: 1e-5 absolute is 40 epsilons of that."""
    c = K.plane_case()
    got = P.gradient(ref, *c["xyz"], c["intensity"], *c["xyz"], *c["normals"], K.R)
    assert got.kmax == 64 and got.neighbors == 64 * 64
    assert np.abs(got.out - np.float32(c["want"])).max() < 1e-5
    # the projection removes what lies along the normal: a tilted normal takes its share out
    n = K.vectors(64, (0.6, 0.0, 0.8))
    tilted = P.gradient(ref, *c["xyz"], c["intensity"], *c["xyz"], *n, K.R).out
    x = np.float64(c["want"])
    nv = np.float64([0.6, 0.0, 0.8])
    assert np.abs(tilted - (x - nv * nv.dot(x))).max() < 1e-5


def test_gradient_special_rows(ref):
    c = K.plane_case()
    xyz, inten, nrm = c["xyz"], c["intensity"], c["normals"]
    # k = 0 (far away, and a non-finite query) and k = 2: NaN rows, written as 0x7fc00000
    two = K.points(K.Q0, K.offset(K.STEP))
    q = K.points((9.0e3, 9.0e3, 9.0e3), (np.nan, 2.0, 3.0), K.Q0)
    got = P.gradient(ref, *two, np.float32([1.0, 2.0]), *q, *K.vectors(3, Z), K.R)
    assert all_nan(got.out) and (got.neighbors, got.kmax) == (2, 2)
    # a NaN normal
    n = tuple(v.copy() for v in nrm)
    n[0][5] = np.nan
    got = P.gradient(ref, *xyz, inten, *xyz, *n, K.R).out
    assert all_nan(got[5]) and np.isfinite(np.delete(got, 5, axis=0)).all()
    # a NaN intensity among the neighbours: the mean is NaN, so every row that sees it is NaN
    i2 = inten.copy()
    i2[9] = np.nan
    assert all_nan(P.gradient(ref, *xyz, i2, *xyz, *nrm, K.R).out)
    # an infinite one is skipped by the second pass, but the mean is infinite: NaN again
    i2[9] = np.inf
    assert all_nan(P.gradient(ref, *xyz, i2, *xyz, *nrm, K.R).out)


def test_gradient_depends_on_the_neighbour_order(ref):
    c = K.order_case()
    a = P.gradient(ref, *c["xyz"], c["intensity"], *c["q"], *c["qnormals"], K.R)
    b = P.gradient(ref, *c["xyz"], c["intensity"], *c["q"], *c["qnormals"], K.R, reversed_order=True)
    assert a.neighbors == 8 * c["k"] and np.isfinite(a.out).all()
    assert (bits(a.out) != bits(b.out)).any(axis=1).sum() >= 6
    assert np.allclose(a.out, b.out, rtol=1e-3, atol=1e-2)


# ---- RIFT ----

def test_rift_parallel_gradient_is_column_zero(ref):
    """ang = acosf(1) = 0: g = 0, weights (0, 1, 0) on the columns -1 (wrapped to G - 1), 0 and 1; the
    zeros are still added.  d = 4 * 2^-6 / (0.05 + eps) = 1.25 (up to rounding): 0.75 in distance bin
    1 and 0.25 in bin 2, normalised by sqrt(0.75^2 + 0.25^2).  The centre's zero gradient adds zeros."""
    xyz, g = K.pair((3.0, 0.0, 0.0))
    got = P.rift(ref, *xyz, *g, *K.points(K.Q0), K.R)
    m = columns(got.out[0])
    assert (got.neighbors, got.kmax) == (2, 2)
    assert not m[1:].any() and m[0, 0] == 0 and m[0, 3] == 0
    want = np.array([0.75, 0.25]) / np.hypot(0.75, 0.25)
    assert np.abs(m[0, 1:3] - want).max() < 1e-5


def test_rift_antiparallel_gradient_wraps_into_column_zero(ref):
    """ang = pi: g = G pi / (pi + eps) is G less an ulp or two, so g_hi = G (or G + 1), and column
    G wraps to column 0 with a weight within 2 ulp(8) ~ 1e-6 of one; what lands in columns G - 1 and
    1 has a weight below that."""
    xyz, g = K.pair((-3.0, 0.0, 0.0))
    m = columns(P.rift(ref, *xyz, *g, *K.points(K.Q0), K.R).out[0])
    want = np.array([0.0, 0.75, 0.25, 0.0]) / np.hypot(0.75, 0.25)
    assert np.abs(m[0] - want).max() < 1e-5
    assert np.abs(m[1:]).max() < 2e-6 and not m[2:7].any()


def test_rift_perpendicular_gradient_is_the_middle_column(ref):
    xyz, g = K.pair((0.0, 0.0, 5.0))
    m = columns(P.rift(ref, *xyz, *g, *K.points(K.Q0), K.R).out[0])
    want = np.array([0.0, 0.75, 0.25, 0.0]) / np.hypot(0.75, 0.25)
    assert np.abs(m[4] - want).max() < 1e-5
    assert np.abs(np.delete(m, 4, axis=0)).max() < 2e-6


def test_rift_special_rows(ref):
    q0 = K.points(K.Q0)
    # only itself as a neighbour: no direction, ang = 0; d = 0 touches distance bins 0 and 1
    # (weights 1 and 0): exactly 1.0 in bin (0, 0)
    got = P.rift(ref, *q0, *K.vectors(1, (0.0, 0.0, 2.0)), *q0, K.R)
    want = np.zeros(32, np.float32)
    want[0] = 1.0
    assert np.array_equal(bits(got.out[0]), bits(want))
    # k = 0: NaN (PCL would leave the previous row)
    far = K.points((9.0e3, 9.0e3, 9.0e3), (np.nan, 2.0, 3.0))
    got = P.rift(ref, *q0, *K.vectors(1, (0.0, 0.0, 2.0)), *far, K.R)
    assert all_nan(got.out) and got.neighbors == 0
    # all-zero gradients: 0 x inf
    xyz, g = K.pair((0.0, 0.0, 0.0))
    assert all_nan(P.rift(ref, *xyz, *g, *q0, K.R).out)
    # one NaN gradient in the ball
    xyz, g = K.pair((1.0, np.nan, 0.0), centre_gradient=(1.0, 2.0, 3.0))
    assert all_nan(P.rift(ref, *xyz, *g, *q0, K.R).out)


@pytest.mark.parametrize("dg", [(4, 1), (4, 2), (1, 1)])
def test_rift_wrapped_columns_collide(ref, dg):
    """G < 3: the columns g_lo .. g_hi wrap onto each other, every weight still lands somewhere, and
    the row has unit norm."""
    D, G = dg
    c = K.order_case(k=40, blobs=2)
    got = P.rift(ref, *c["xyz"], *c["gradients"], *c["q"], K.R, D, G)
    assert got.out.shape == (2, D * G) and np.isfinite(got.out).all()
    assert np.abs(np.linalg.norm(got.out.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_rift_depends_on_the_neighbour_order(ref):
    c = K.order_case()
    a = P.rift(ref, *c["xyz"], *c["gradients"], *c["q"], K.R)
    b = P.rift(ref, *c["xyz"], *c["gradients"], *c["q"], K.R, reversed_order=True)
    assert a.neighbors == 8 * c["k"] and np.isfinite(a.out).all()
    assert (bits(a.out) != bits(b.out)).any(axis=1).sum() >= 6
    assert np.allclose(a.out, b.out, rtol=1e-4, atol=1e-6)


# ---- Eigen 3.2's float sum ----

def test_eigen_float_sum_follows_the_stated_rule(ref):
    rng = np.random.default_rng(5)
    differs = 0
    for n in list(range(1, 41)) + [255, 256]:   # every tail: n mod 8, below and above one packet pair
        m = (rng.uniform(0.0, 1.0, n) ** 2).astype(np.float32)
        got, want = P.eigen_sum(ref, m), P.eigen_sum_py(m)
        assert bits(got).item() == bits(want).item(), n
        differs += int(bits(got).item() != bits(P.sequential_sum(m)).item())
    assert differs > 10   # it is not the sequential sum
