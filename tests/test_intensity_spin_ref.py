"""The CPU restatement of the intensity spin images (tests/cpp/intensity_spin_ref.cpp) pinned by
contract, not by itself: closed-form rows, the special rows of pfx.h, and the proof that the neighbour
order decides bits (so the GPU comparison of tests/test_gpu_intensity_spin.py has teeth)."""
import math

import numpy as np
import pytest

import intensity_spin_cases as K
import intensity_spin_ref as P
from parity import bits


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("intensity_spin_ref"))


def all_nan(row):
    return (bits(row) == K.NAN_BITS).all()


def ulps_apart(a, b):
    """Of positive finite floats."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def test_lone_point_is_the_gaussian_at_the_origin(ref):
    """d = i = 0 and c = 1/2: every argument -(dj^2 + ii^2) / 2 is exact in float32, so a weight is
    pfx_expf of the very number math.exp gets, and two faithful roundings of one value are at most
    1 ulp apart.  The window is [0, 3] on both axes: the bins with ii = 4 are never touched."""
    xyz, inten = K.lone()
    got = P.spin(ref, *xyz, inten, *xyz, K.R)
    assert (got.neighbors, got.kmax) == (1, 1) and got.out.shape == (1, 20)
    m = got.out[0].reshape(4, 5)
    want = np.float32([[math.exp(-(dj * dj + ii * ii) / 2.0) for ii in range(4)] for dj in range(4)])
    assert ulps_apart(m[:, :4], want).max() <= 1
    assert m[0, 0] == 1.0 and (bits(m[:, 4]) == 0).all()


def test_hand_computed_pair(ref):
    """Centre (d, i) = (0, 0) and the neighbour (pair_d, I): the darker intensity is the minimum and
    the brighter has i == I exactly.  Against the double-precision image: an argument is at most
    (3^2 + 5^2) / 2 = 17 in magnitude and comes from four float roundings (a a, its product with c, b b
    c, the difference), 17 * 4 * 2^-24 = 4e-6 absolute, which is the relative error of the weight; the
    exponential's ulp and the addition's add 1.2e-7: 1e-5 relative bounds them."""
    xyz, inten = K.pair()
    got = P.spin(ref, *xyz, inten, *K.points(K.Q0), K.R)
    assert (got.neighbors, got.kmax) == (2, 2)
    d1 = float(K.pair_d())
    assert abs(d1 - 1.25) < 1e-5
    want = K.gauss_image([(0.0, 0.0), (d1, 5.0)])
    assert np.abs(got.out[0] / want - 1.0).max() < 1e-5
    # the other order of intensities: the centre is the brighter one
    got = P.spin(ref, *xyz, inten[::-1].copy(), *K.points(K.Q0), K.R)
    assert np.abs(got.out[0] / K.gauss_image([(0.0, 5.0), (d1, 0.0)]) - 1.0).max() < 1e-5


def test_sigma_zero_rows_are_counts_and_drop_the_brightest(ref):
    """sigma == 0: every neighbour adds 1 to one bin.  The brightest neighbour has i == I and PCL
    would write past the image: here it is dropped, so the row sums to k - 1."""
    xyz, inten = K.ramp_blob()
    q = K.points(K.Q0)
    got = P.spin(ref, *xyz, inten, *q, K.R, sigma=0.0)
    row = got.out[0]
    assert got.kmax == 256 and np.array_equal(row, np.round(row)) and row.sum() == 255
    # the intensity bins of 0 .. 254 over 255: 51 each
    assert np.array_equal(row.reshape(4, 5).sum(axis=0), [51, 51, 51, 51, 51])
    xyz, inten = K.pair()
    got = P.spin(ref, *xyz, inten, *q, K.R, sigma=0.0)
    want = np.zeros(20, np.float32)
    want[0] = 1.0   # the centre in bin (0, 0); the neighbour, i == I, dropped
    assert np.array_equal(bits(got.out[0]), bits(want))


def test_a_nan_intensity_is_ignored(ref):
    xyz, inten = K.pair()
    three = K.points(K.Q0, K.offset(0.0, K.STEP / 2), K.offset(K.STEP))
    i3 = np.float32([inten[0], np.nan, inten[1]])
    q = K.points(K.Q0)
    for sigma in (1.0, 0.0):
        a = P.spin(ref, *xyz, inten, *q, K.R, sigma=sigma)
        b = P.spin(ref, *three, i3, *q, K.R, sigma=sigma)
        assert b.kmax == 3 and np.array_equal(bits(a.out), bits(b.out))


def test_all_nan_intensities_give_a_zero_row(ref):
    xyz, inten = K.pair(np.nan, np.nan)
    for sigma in (1.0, 0.0):
        got = P.spin(ref, *xyz, inten, *K.points(K.Q0), K.R, sigma=sigma)
        assert got.kmax == 2 and (bits(got.out) == 0).all()


def test_no_neighbour_is_a_nan_row(ref):
    xyz, inten = K.pair()
    got = P.spin(ref, *xyz, inten, *K.points(K.FAR, (np.nan, 2.0, 3.0)), K.R)
    assert all_nan(got.out) and got.neighbors == 0


def test_an_overflowing_range_contributes_nothing(ref):
    """I (I_n - min) overflows to infinity: i is no number a window can be cast from, and the
    neighbour is skipped; the darker one lands at i = 0."""
    xyz, inten = K.pair(0.0, 3.0e38)
    got = P.spin(ref, *xyz, inten, *K.points(K.Q0), K.R)
    want = K.gauss_image([(0.0, 0.0)])
    hit = want > 0
    assert hit.sum() == 16 and np.abs(got.out[0][hit] / want[hit] - 1.0).max() < 1e-5
    assert (bits(got.out[0][~hit]) == 0).all()


def test_depends_on_the_neighbour_order(ref):
    c = K.order_case()
    a = P.spin(ref, *c["xyz"], c["intensity"], *c["q"], K.R)
    b = P.spin(ref, *c["xyz"], c["intensity"], *c["q"], K.R, reversed_order=True)
    assert a.neighbors == 8 * c["k"] and np.isfinite(a.out).all()
    assert (bits(a.out) != bits(b.out)).any(axis=1).sum() >= 6
    assert np.allclose(a.out, b.out, rtol=1e-4, atol=1e-6)
