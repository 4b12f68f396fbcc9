"""Closed forms that pin the CPU restatement of the boundary contract (tests/cpp/boundary_ref.cpp,
DESIGN.md "Boundary: the contract"), which the kernel is then compared with bit for bit
(tests/test_gpu_boundary.py).  No GPU."""
import math

import numpy as np
import pytest

import boundary_cases as K
import boundary_ref as P

PI = math.pi


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("boundary_ref"))


def flag(ref, case, t=PI / 2, r=K.R):
    s, q, n = case
    return int(P.flags(ref, *s, *q, *n, r, t).flags[0])


def test_lattice_rim_and_interior(ref):
    xyz, nrm, rim = K.lattice()
    got = P.flags(ref, *xyz, *xyz, *nrm, 0.025)
    assert rim.sum() == 32 and np.array_equal(got.flags, rim.astype(np.uint8))
    assert got.flagged == 32 and got.kmax == 21 and got.neighbors == int(got.k.sum())
    # an interior point's largest gap is 45 degrees at the most (beside the rim; atan(1 / 2) deeper in),
    # a corner's 270 and an edge's 180
    gap = np.degrees(got.max_gap.astype(np.float64))
    assert gap[~rim].max() < 45.001 and abs(gap[~rim].min() - math.degrees(math.atan(0.5))) < 1e-3
    assert sorted(set(np.round(gap[rim]).astype(int).tolist())) == [180, 270]


def test_ring_of_equally_spaced_points(ref):
    assert flag(ref, K.ring(K.even(3))) == 1      # gaps of 120 degrees
    assert flag(ref, K.ring(K.even(5))) == 0      # 72
    got = P.flags(ref, *K.ring(K.even(3))[0], *K.ring(K.even(3))[1], *K.ring(K.even(3))[2], K.R)
    assert abs(float(got.max_gap[0]) - 2 * PI / 3) < 1e-5 and got.k[0] == 4


def test_counts(ref):
    far = K.points((9.0, 9.0, 9.0))
    s, q, n = K.ring(K.even(1))
    assert flag(ref, (s, q, n)) == 0 and P.flags(ref, *s, *q, *n, K.R).k[0] == 2     # k = 2
    assert flag(ref, (s, far, n)) == 255                                           # no neighbour
    assert flag(ref, (s, K.points((np.nan, 0.0, 0.0)), n)) == 255                  # a non-finite query
    only = K.ring([], duplicates=3)
    assert flag(ref, only) == 0 and P.flags(ref, *only[0], *only[1], *only[2], K.R).k[0] == 4    # cp = 0
    one = K.ring([1.0], duplicates=3)
    got = P.flags(ref, *one[0], *one[1], *one[2], K.R, 6.2)
    # cp = 1: the wrap term, (2 pi - a) + a, above every threshold that can be asked for
    assert got.flags[0] == 1 and abs(float(got.max_gap[0]) - 2 * PI) < 1e-6
    # a query that is no surface point counts no copy of itself
    s, q, n = K.ring(K.even(3), with_centre=False)
    assert P.flags(ref, *s, *q, *n, K.R).k[0] == 3 and flag(ref, (s, q, n)) == 1
    # non-finite surface points are nobody's neighbours
    s, q, n = K.ring(K.even(5))
    bad = tuple(np.append(v, np.float32(w)) for v, w in zip(s, (np.nan, 0.0, np.inf)))
    assert P.flags(ref, *bad, *q, *n, K.R).k[0] == 6


@pytest.mark.parametrize("bad", [(np.nan, 0.0, 1.0), (0.0, 0.0, np.nan), (0.0, 0.0, 0.0), (np.inf, 0.0, 1.0),
                                 (0.0, -np.inf, 0.0)], ids=str)
def test_unusable_normals_give_0(ref, bad):
    s, q, _ = K.ring(K.even(3))
    assert flag(ref, (s, q, K.points((0.0, 0.0, 1.0)))) == 1
    assert flag(ref, (s, q, K.points(bad))) == 0


@pytest.mark.parametrize("name", sorted(K.NORMALS))
def test_every_branch_of_the_axes(ref, name):
    """The ring laid in the plane of each normal: both choices of s, every m, the ties.  The flags are
    the unrotated ring's, and the axes are orthonormal and orthogonal to n."""
    n = K.NORMALS[name]
    u, v = (a.astype(np.float64) for a in K.plane_axes(n))
    nn = np.asarray(n) / np.linalg.norm(n)
    assert abs(u @ v) < 1e-6 and abs(v @ nn) < 1e-6 and abs(u @ nn) < 1e-6 and abs(np.linalg.norm(v) - 1) < 1e-6
    want_m = {"x": 0, "y": 1, "z": 2, "tie_xy": 0, "tie_yz": 1, "tie_all": 0, "minus_z": 2}[name]
    zero = {0: 2, 1: 2, 2: 1}[want_m]     # v has components m and s only
    assert K.plane_axes(n)[1][zero] == 0
    for m, want in ((3, 1), (5, 0)):
        assert flag(ref, K.ring(K.even(m), n=n, centre=(0.3, -0.2, 0.1))) == want, (name, m)
    # half a ring is a boundary in any plane
    assert flag(ref, K.ring(np.linspace(-1.5, 1.5, 9), n=n)) == 1


def test_wrap_term(ref):
    d = math.radians
    # a 60 degree fan across the +-pi cut: its angles lie at both ends of the sorted array
    fan = K.ring([PI - d(30), PI - d(10), -PI + d(10), -PI + d(30)])
    got = P.flags(ref, *fan[0], *fan[1], *fan[2], K.R)
    assert got.flags[0] == 1 and abs(float(got.max_gap[0]) - d(300)) < 1e-5
    # a full ring every 20 degrees, but 80 across the cut: only the wrap term sees the thin spot
    thin = K.ring(np.radians(np.arange(-140, 141, 20)))
    got = P.flags(ref, *thin[0], *thin[1], *thin[2], K.R)
    assert got.flags[0] == 0 and abs(float(got.max_gap[0]) - d(80)) < 1e-5
    assert flag(ref, thin, t=d(79)) == 1 and flag(ref, thin, t=d(81)) == 0
    # ... and 100 degrees across the cut is a boundary by the wrap term alone
    wide = K.ring(np.radians(np.arange(-130, 131, 20)))
    assert flag(ref, wide) == 1 and flag(ref, wide, t=d(101)) == 0


def test_angles_at_the_ends_of_the_range(ref):
    pts, r = K.bin_edge_angles()
    origin, up = K.points((0.0, 0.0, 0.0)), K.points((0.0, 0.0, 1.0))
    for a, b, gap in (("+pi", "-pi", 2 * K.PI_F), ("+0", "-0", 2 * K.PI_F), ("+pi", "+0", K.PI_F),
                      ("-pi", "-0", K.PI_F)):
        s = K.points((0.0, 0.0, 0.0), pts[a], pts[b])
        got = P.flags(ref, *s, *origin, *up, r, 3.0)
        assert got.k[0] == 3 and got.max_gap[0] == np.float32(gap), (a, b)
    s = K.points((0.0, 0.0, 0.0), *pts.values())
    got = P.flags(ref, *s, *origin, *up, r, 3.0)
    assert got.flags[0] == 1 and got.max_gap[0] == K.PI_F
    assert P.flags(ref, *s, *origin, *up, r, 3.15).flags[0] == 0


def test_shuffling_the_surface_changes_nothing(ref):
    xyz = K.holed_plane(n=600, seed=3)
    nrm = K.f32(np.zeros(600), np.zeros(600), np.ones(600))
    want = P.flags(ref, *xyz, *xyz, *nrm, 0.1)
    assert 0 < want.flagged < 600
    perm = np.random.default_rng(4).permutation(600)
    got = P.flags(ref, *(v[perm] for v in xyz), *xyz, *nrm, 0.1)
    assert np.array_equal(got.flags, want.flags) and np.array_equal(got.max_gap, want.max_gap)
    assert (got.neighbors, got.kmax, got.flagged) == (want.neighbors, want.kmax, want.flagged)


def test_flags_are_monotone_in_the_threshold(ref):
    xyz = K.holed_plane(n=600, seed=5)
    nrm = K.f32(np.zeros(600), np.zeros(600), np.ones(600))
    rows = [P.flags(ref, *xyz, *xyz, *nrm, 0.1, t).flags for t in (PI / 4, PI / 2, PI, 3.0)]
    # (pi > 3: the thresholds ascend as pi / 4, pi / 2, 3, pi)
    order = [rows[0], rows[1], rows[3], rows[2]]
    for lo, hi in zip(order, order[1:]):
        assert (hi <= lo).all()
    assert rows[0].sum() > rows[2].sum() > 0
