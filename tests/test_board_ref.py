"""The CPU restatement of the BOARD frames (tests/cpp/board_ref.cpp) pinned by contract, not by
itself: closed-form rows on surfaces whose centroid and sums are exact (tests/board_cases.py), the
NaN rules, and the proof that the neighbour order decides bits, so that the GPU comparison of
tests/test_gpu_board.py has teeth.  A claimed row states no sign for a zero: -0 and +0 are one
value here, every other float is compared in its bits."""
import numpy as np
import pytest

import board_cases as K
import board_ref as P
from parity import bits

FAR = (9.0e3, 9.0e3, 9.0e3)
C_R = 0.05  # the radius of the blobs of pfh_cases
CASES = K.closed_form_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("board_ref"))


def all_nan(rows):
    return (bits(rows) == K.NAN_BITS).all()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_closed_form_rows(ref, case):
    _, xyz, nrm, tangent_radius, row = case
    got = P.frames(ref, *xyz, *nrm, *K.points(K.Q0), K.R, tangent_radius)
    assert got.kmax == len(xyz[0])                       # every point of a case is a neighbour of Q0
    assert np.array_equal(K.got_bits(got.rf[0]), K.row_bits(row)), (got.rf[0], row)
    # the sums are exact, so the walk's direction changes nothing
    rev = P.frames(ref, *xyz, *nrm, *K.points(K.Q0), K.R, tangent_radius, reversed_order=True)
    assert np.array_equal(bits(rev.rf), bits(got.rf))


def test_the_cases_are_what_they_say():
    """The geometry behind the claims, stated in numpy: exact centroids, the rings, the ties."""
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names) == 15
    for _, xyz, _, _, _ in CASES[:11]:                   # (the k = 5 case drops a point of a balanced set)
        k = len(xyz[0])
        assert [float(np.sum(v, dtype=np.float64)) for v in xyz] == [k * 1.0, k * 2.0, k * 3.0]
    m_r = (np.float32(0.85) * np.float32(0.85)) * (np.float32(K.R) * np.float32(K.R))
    m_t = (np.float32(0.85) * np.float32(0.85)) * (np.float32(K.TR) * np.float32(K.TR))
    h2 = K.H * K.H
    assert 64 * h2 < m_r < 196 * h2 < K.R * K.R and 25 * h2 < m_t < 49 * h2 < K.TR * K.TR < 144 * h2
    xyz, _ = K.patch(K.TWINS)
    nb, d2 = K.flann_order(xyz, K.Q0, K.R * K.R)
    assert nb[:3].tolist() == [0, 1, 2] and d2[1] == d2[2] == np.float32(4 * h2)
    xyz, _ = K.patch(K.BASE)
    nb, d2 = K.flann_order(xyz, K.Q0, K.R * K.R)
    assert nb[:2].tolist() == [0, 1] and d2[1] < d2[2]


def test_chosen_neighbours(ref):
    """Which neighbour gives x, read back from the restatement."""
    by_name = {c[0]: c for c in CASES}
    for name, want in (("unique nearest neighbour", 1), ("two nearest neighbours, the lower index wins", 1),
                       ("one tilted normal", K.TILTED_ROW),
                       ("tilted normal inside the margin, neighbours in the ring", 7),
                       ("tilted normal inside the margin, empty ring", K.TILTED_ROW),
                       ("tilted normal between the radii is ignored for x", 3),
                       ("... and decides x with the tangent radius unset", 7),
                       ("one NaN normal: no flip, never chosen", 2), ("all normals NaN", -1), ("k = 5", -1)):
        _, xyz, nrm, tangent_radius, _ = by_name[name]
        assert P.frames(ref, *xyz, *nrm, *K.points(K.Q0), K.R, tangent_radius).chosen[0] == want, name


def test_a_margin_neighbour_with_a_nan_normal_blocks_the_fallback(ref):
    """Tangent radius R, the ring holds one neighbour and its normal is NaN: a margin point was found,
    so the scan over the inner neighbours is not run and the row is NaN; without that neighbour the
    fallback finds the tilted normal."""
    ring = K.BASE + ((14, 0), (-14, 0))
    xyz, nrm = K.patch(ring, special={7: K.NAN3, 8: K.NAN3, K.TILTED_ROW: K.TILT})
    got = P.frames(ref, *xyz, *nrm, *K.points(K.Q0), K.R, K.R)
    assert all_nan(got.rf) and got.chosen[0] == -1
    xyz, nrm = K.patch(K.BASE, special={K.TILTED_ROW: K.TILT})
    assert P.frames(ref, *xyz, *nrm, *K.points(K.Q0), K.R, K.R).chosen[0] == K.TILTED_ROW


def test_margin_threshold(ref):
    """margin_thresh = 0 puts every neighbour with d2 > 0 on the margin of any tangent radius;
    margin_thresh = 1 nobody (d2 < r^2 is strict), so the fallback runs over all, the centre first:
    with equal normals the centre itself is chosen and x is 0 / 0."""
    xyz, nrm = K.patch(K.BASE)
    q = K.points(K.Q0)
    got = P.frames(ref, *xyz, *nrm, *q, K.R, K.R, margin_thresh=0.0)
    assert got.chosen[0] == 1 and np.array_equal(K.got_bits(got.rf[0]), K.row_bits(K.X_POS))
    got = P.frames(ref, *xyz, *nrm, *q, K.R, K.R, margin_thresh=1.0)
    assert got.chosen[0] == 0 and np.array_equal(K.got_bits(got.rf[0]), K.row_bits((np.nan,) * 6 + (0, 0, 1)))


def test_special_queries(ref):
    xyz, nrm = K.patch(K.BASE)
    q = K.points(K.Q0, FAR, (np.nan, 2.0, 3.0), (1.0, np.inf, 3.0))
    got = P.frames(ref, *xyz, *nrm, *q, K.R)
    assert np.isfinite(got.rf[0]).all() and all_nan(got.rf[1:])
    assert got.k.tolist() == [7, 0, 0, 0] and (got.neighbors, got.kmax) == (7, 7)
    # a non-finite surface point is nobody's neighbour
    x = np.append(xyz[0], np.float32(np.nan))
    s = (x, np.append(xyz[1], np.float32(2.0)), np.append(xyz[2], np.float32(3.0)))
    n = tuple(np.append(v, np.float32(1.0)) for v in nrm)
    got = P.frames(ref, *s, *n, *K.points(K.Q0), K.R)
    assert got.kmax == 7 and np.isfinite(got.rf).all()
    # no surface at all
    none = tuple(v[:0] for v in xyz)
    got = P.frames(ref, *none, *none, *K.points(K.Q0), K.R)
    assert all_nan(got.rf) and (got.neighbors, got.kmax) == (0, 0)


def test_the_gathered_count_is_that_of_the_larger_radius(ref):
    """The statistics count the neighbours at max(r, tangent_radius)."""
    xyz, nrm = K.patch(K.BASE + ((14, 0), (-14, 0)))
    q = K.points(K.Q0)
    assert P.frames(ref, *xyz, *nrm, *q, K.TR, K.R).k[0] == 9       # r = TR reaches 6, the tangent radius all 9
    assert P.frames(ref, *xyz, *nrm, *q, K.TR).k[0] == 6            # ((8, 0) lies at TR exactly: d2 < r^2 is strict)
    assert P.frames(ref, *xyz, *nrm, *q, K.R, K.TR).k[0] == 9


def test_against_a_float64_statement_on_random_blobs(ref):
    """z is the direction of least variance, towards the mean normal; x lies in its plane and points
    at the projection of the chosen neighbour; the frame is orthonormal.  Within 1e-4."""
    c = K.order_case(k=120, blobs=4)
    got = P.frames(ref, *c["xyz"], *c["normals"], *c["q"], C_R)
    s = np.stack(c["xyz"], 1).astype(np.float64)
    n = np.stack(c["normals"], 1).astype(np.float64)
    for i, row in enumerate(got.rf.astype(np.float64)):
        p = np.array([v[i] for v in c["q"]], np.float64)
        nb, _ = K.flann_order(c["xyz"], p, C_R * C_R)
        a = s[nb] - s[nb].mean(axis=0)
        w, v = np.linalg.eigh(a.T @ a)
        z = v[:, 0] * (1.0 if v[:, 0] @ n[nb].sum(axis=0) >= 0 else -1.0)
        assert np.abs(row[6:] - z).max() < 1e-4
        cos = n[nb[1:]] @ z                     # the centre itself (d2 = 0) is not on the margin
        b = s[nb[1:][int(np.argmin(cos))]]
        assert nb[1:][int(np.argmin(cos))] == got.chosen[i]
        x = (b - (z @ (b - p)) * z) - p
        x /= np.linalg.norm(x)
        assert np.abs(row[:3] - x).max() < 1e-4 and np.abs(row[3:6] - np.cross(z, x)).max() < 1e-4


def test_the_neighbour_order_decides_bits(ref):
    c = K.order_case()
    fwd = P.frames(ref, *c["xyz"], *c["normals"], *c["q"], C_R)
    rev = P.frames(ref, *c["xyz"], *c["normals"], *c["q"], C_R, reversed_order=True)
    assert fwd.kmax == c["k"] and np.isfinite(fwd.rf).all()
    assert (bits(fwd.rf) != bits(rev.rf)).any()


def test_the_tie_case_picks_the_first_of_the_tied(ref):
    xyz, nrm, q, nb, first = K.tie_case()
    got = P.frames(ref, *xyz, *nrm, *q, C_R)
    assert got.chosen[0] == nb[first] and np.isfinite(got.rf).all()
    z = got.rf[0, 6:]
    cos = (z[0] * nrm[0] + z[1] * nrm[1]) + z[2] * nrm[2]
    assert len(np.unique(cos[nb[first:]])) == 1 and cos[nb[first]] < cos[nb[:first]].min()

