"""The CPU restatement (oracle/) against the float64 statements of normals, FPFH-33 and SHOT-352
(tests/f64_ref.py) on the clouds of tests/f64_cases.py -- CPU only.

(a) the restatement lies within the bounds of tests/f64_check.py on every case (the figures are
    printed: pytest -s); (b) the statements are sharp: each of eleven planted errors -- a wrong
    reading of the definition of the kind a restatement and a kernel written from it would share
    -- fails (a) on at least 90 % of the finite rows; (c) the statements themselves reproduce
    analytic answers, so they are not one more unpinned reading.

One planted error cannot fail on 90 % of all rows: "SHOT's x axis left unflipped" is the correct
frame wherever the eigenvector came out of the solver on the majority's side already (about half
of the rows, by the solver's arbitrary sign).  Its share is taken over the rows where the
unflipped frame differs from the flipped one, and those must be at least a quarter of the rows.
"""
import numpy as np
import pytest

import f64_cases as C
import f64_check as K
import f64_ref as R
import oracle_lib as O


def _show(name, fig):
    print("\n%s: %s" % (name, ", ".join("%s %.3g" % kv for kv in fig.items())))


# ---- (a) the restatement within the bounds ---------------------------------------------------

@pytest.mark.parametrize("case", [C.surface_origin, C.surface_range], ids=lambda f: f.__name__)
def test_restated_normals_within_the_derived_bound(case):
    fig, _ = K.run_normals(O, case())
    _show(case.__name__ + " (worst angle, rad)", fig)


@pytest.mark.parametrize("case", [C.rough_blob, C.rough_blob_keypoints], ids=lambda f: f.__name__)
def test_restated_fpfh_within_its_interval(case):
    fig, got = K.run_fpfh(O, case())
    _show(case.__name__, fig)
    if case is C.rough_blob_keypoints:
        assert np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()


@pytest.mark.parametrize("case", [C.aniso_blob, C.dense_core], ids=lambda f: f.__name__)
def test_restated_shot_frame_and_descriptor(case):
    fig, _ = K.run_shot(O, case())
    _show(case.__name__, fig)


def test_restated_chain_normals_fpfh_shot():
    fig, _ = K.run_chain(O, C.surface_chain())
    for stage, f in fig.items():
        _show("surface_chain " + stage, f)


# ---- (b) the statements are sharp ------------------------------------------------------------

@pytest.fixture(scope="module")
def fpfh_got():
    c = C.rough_blob()
    return c, np.asarray(O.fpfh(*K.xyz(c.P), *K.xyz(c.N), *K.xyz(c.Q), c.r, False))


@pytest.fixture(scope="module")
def shot_got():
    c = C.aniso_blob()
    return (c,) + tuple(O.shot(*K.xyz(c.P), *K.xyz(c.N), *K.xyz(c.Q), c.r))


def _fpfh_rejected(ref, got):
    fin = np.isfinite(ref.lo).all(1)
    return (K.fpfh_excess(ref, got)[fin] > K.S_FPFH).mean()


def test_fpfh_unplanted_passes(fpfh_got):
    c, got = fpfh_got
    assert _fpfh_rejected(c.ref, got) == 0.0


@pytest.mark.parametrize("name", ["row rolled by one bin", "f2 and f3 blocks exchanged"])
def test_fpfh_error_planted_in_the_output_is_rejected(fpfh_got, name):
    c, got = fpfh_got
    if name == "row rolled by one bin":
        bad = np.roll(got, 1, axis=1)
    else:
        bad = np.concatenate([got[:, :11], got[:, 22:], got[:, 11:22]], 1)
    share = _fpfh_rejected(c.ref, bad)
    print("\n%s: rejected on %.0f %% of the rows" % (name, 100 * share))
    assert share >= K.SHARP


@pytest.mark.parametrize("name, conv", [
    ("swap rule removed", dict(swap_rule=False)),
    ("weights 1/d instead of 1/d^2", dict(weight_power=1)),
    ("increment 100/k instead of 100/(k-1)", dict(incr_minus=0)),
    ("self pair not skipped", dict(skip_self=False)),
])
def test_fpfh_error_planted_in_the_statement_is_rejected(fpfh_got, name, conv):
    from types import SimpleNamespace
    c, got = fpfh_got
    lo, hi, share = R.fpfh_interval(c.P, c.N, c.Q, c.r, False, C.TAU, conv)
    rejected = _fpfh_rejected(SimpleNamespace(lo=lo, hi=hi), got)
    print("\n%s: rejected on %.0f %% of the rows" % (name, 100 * rejected))
    assert rejected >= K.SHARP


def _shot_rejected(c, desc, rf, conv, frame):
    """Share of the compared rows on which the restatement misses the statement with `conv`
    planted; frame: the error is in the frame (else in the histogram, compared in the product's
    own frame).  Also returns the share of rows on which the planted statement differs at all."""
    use = K.shot_compared_rows(c.ref)
    if frame:
        bad_rf = np.array([R.shot_lrf(c.P, q, c.r, conv)[0] for q in c.Q])
        differs = use & (np.abs(bad_rf - c.ref.rf).max(1) > 0)
        miss = np.abs(rf.astype(np.float64) - bad_rf).max(1) > K.T_RF
    else:
        bad = np.array([R.shot352(c.P, c.N, q, f, c.r, conv) for q, f in zip(c.Q, rf)])
        differs = use & (np.abs(bad - K.shot_own_frame(c, rf)).max(1) > 0)
        miss = np.linalg.norm(desc.astype(np.float64) - bad, axis=1) > K.T_DESC
    return miss[use].mean(), miss[differs].mean() if differs.any() else 0.0, differs.sum() / use.sum()


def test_shot_unplanted_passes(shot_got):
    c, desc, rf = shot_got
    assert _shot_rejected(c, desc, rf, None, True)[0] == 0.0
    assert _shot_rejected(c, desc, rf, None, False)[0] == 0.0


@pytest.mark.parametrize("name, conv, frame", [
    ("azimuth side bin at sel +- 2", dict(azimuth_side=2), False),
    ("radial knot at r/3", dict(radial_knot=1.0 / 3.0), False),
    ("cosine bins wrapped modulo 11", dict(cosine_wrap=11), False),
    ("(r - d) weights dropped from the frame", dict(lrf_weighted=False), True),
])
def test_shot_planted_error_is_rejected(shot_got, name, conv, frame):
    c, desc, rf = shot_got
    rejected, _, _ = _shot_rejected(c, desc, rf, conv, frame)
    print("\n%s: rejected on %.0f %% of the rows" % (name, 100 * rejected))
    assert rejected >= K.SHARP


def test_shot_x_axis_left_unflipped_is_rejected(shot_got):
    """Over the rows where the planted error changes the frame (module docstring)."""
    c, desc, rf = shot_got
    overall, rejected, present = _shot_rejected(c, desc, rf, dict(flip_x=False), True)
    print("\nx axis left unflipped: present on %.0f %% of the rows, rejected on %.0f %% of those (%.0f %% of all)"
          % (100 * present, 100 * rejected, 100 * overall))
    assert present >= 0.25
    assert rejected >= K.SHARP


# ---- (c) analytic answers for the statements themselves ----------------------------------------

def test_neighbours_are_strict_ordered_and_report_their_margin():
    P = np.array([[0, 0, 0], [0.5, 0, 0], [-0.25, 0, 0], [0.25, 0, 0], [0.4, 0, 0]], np.float32)
    idx, d, margin = R.neighbours(P, P[0], 0.5)
    assert list(idx) == [0, 2, 3, 4]               # d = r is outside; ties by index
    assert np.allclose(d, [0, 0.25, 0.25, 0.4], atol=1e-7)
    assert margin == 0.0
    assert np.isclose(R.neighbours(P[[0, 2, 3, 4]], P[0], 0.5)[2], (0.25 - np.float64(np.float32(0.4)) ** 2) / 0.25)
    assert len(R.neighbours(P, [np.nan, 0, 0], 0.5)[0]) == 0


def test_normals_of_a_plane_are_exact():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12)), -1).reshape(-1, 2) / 128.0
    P = np.c_[g, g[:, 0] + g[:, 1]].astype(np.float32)          # z = x + y, exact in float32
    got = R.normals(P, 0.03, (0.0, 0.0, -5.0))
    assert np.allclose(got.n, np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0), atol=1e-12)
    assert np.abs(got.curvature).max() < 1e-13
    assert np.allclose(R.normals(P, 0.03, (0.0, 0.0, 5.0)).n, np.array([-1.0, -1.0, 1.0]) / np.sqrt(3.0), atol=1e-12)
    assert got.k.min() >= 3 and np.all(got.gap > 0)
    lone = np.r_[P, [[5.0, 5.0, 5.0], [5.0, 5.001, 5.0]]].astype(np.float32)
    out = R.normals(lone, 0.03)
    assert np.isnan(out.n[-2:]).all() and np.isnan(out.curvature[-2:]).all() and np.isfinite(out.n[:-2]).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_normals_of_a_sphere_are_radial(axis):
    # the pole of a sphere of radius 0.5 with three rings of twelve points around it: by symmetry
    # the normal at the pole is the radius; the viewpoint is the centre, so it points inwards
    az = np.arange(12) * (2.0 * np.pi / 12.0)
    pts = [[0.0, 0.0, 0.5]]
    for polar in (0.02, 0.04, 0.05):
        pts += [[0.5 * np.sin(polar) * np.cos(a + polar), 0.5 * np.sin(polar) * np.sin(a + polar), 0.5 * np.cos(polar)]
                for a in az]
    P = np.roll(np.array(pts), axis + 1, axis=1).astype(np.float32)
    got = R.normals(P, 0.03, (0.0, 0.0, 0.0))
    assert got.k[0] == 37
    want = -P[0].astype(np.float64) / 0.5
    assert np.abs(got.n[0] - want).max() < 1e-6      # (the float32 coordinates break the symmetry by 1e-7)
    assert 0 < got.curvature[0] < 0.01


def test_pair_features_reproduce_a_hand_computed_pair():
    # dp = (0.3, 0, 0.4), |dp| = 0.5.  a1 = n1 . dp / 0.5 = 0.224, a2 = n2 . dp / 0.5 = 0.8:
    # acos 0.224 > acos 0.8, so the pair is swapped: u = n2 = z, target normal n1, dp negated,
    # f3 = -a2 = -0.8;  v = (-dp) x u / |.| = (0, 1, 0);  w = u x v = (-1, 0, 0);
    # f2 = v . n1 = 0.6;  f1 = atan2(w . n1, u . n1) = atan2(0.48, 0.64) = atan 0.75.
    p1, n1 = [0.0, 0.0, 0.0], [-0.48, 0.6, 0.64]
    p2, n2 = [0.3, 0.0, 0.4], [0.0, 0.0, 1.0]
    f1, f2, f3, ok, (swap_margin, v_sine, theta_radius) = R.pair_features(p1, n1, p2, n2)
    assert ok[0]
    assert np.isclose(f1[0], np.arctan(0.75), atol=1e-15) and np.isclose(f2[0], 0.6, atol=1e-15)
    assert np.isclose(f3[0], -0.8, atol=1e-15)
    assert np.isclose(swap_margin[0], 0.8 - 0.224, atol=1e-15)
    assert np.isclose(v_sine[0], 0.6, atol=1e-15)            # |dp x z| / |dp| = 0.3 / 0.5
    assert np.isclose(theta_radius[0], 0.8, atol=1e-15)      # hypot(0.48, 0.64)
    # seen from the other point no swap is needed and the features are the same
    g = R.pair_features(p2, n2, p1, n1)
    assert np.allclose([g[0][0], g[1][0], g[2][0]], [f1[0], f2[0], f3[0]], atol=1e-15)
    # without the rule: u = n1, f3 = a1
    h = R.pair_features(p1, n1, p2, n2, dict(swap_rule=False))
    assert np.isclose(h[2][0], 0.224, atol=1e-15) and not np.isclose(h[1][0], 0.6, atol=1e-3)
    # the failure returns: coincident points, and dp parallel to the source normal
    for q2, m2 in ((p1, n2), ([0.0, 0.0, 0.5], n2)):
        f = R.pair_features(p1, [0.0, 0.0, 1.0], q2, m2)
        assert not f[3][0] and f[0][0] == f[1][0] == f[2][0] == 0.0


def test_fpfh_interval_of_a_hand_computed_cloud():
    # four points, all within r of each other, so every SPFH has k = 4, three pairs of 100 / 3 each;
    # the FPFH of point 0 is the 1 / d^2 mean of the SPFHs of points 1 .. 3, every block scaled to 100
    P = np.array([[0, 0, 0], [0.01, 0.002, 0.003], [-0.004, 0.02, 0.001], [0.002, -0.003, 0.03]], np.float32)
    N = np.array([[0, 0, 1], [0, 0.6, 0.8], [0.6, 0, 0.8], [0.28, 0.0, 0.96]], np.float32)
    lo, hi, share = R.fpfh_interval(P, N, P[:1], 0.1, False, C.TAU)
    assert share[0] < 1e-9 and np.allclose(lo, hi)
    assert np.allclose(lo[0].reshape(3, 11).sum(1), 100.0, atol=1e-12)
    want = np.zeros(33)
    wsum = 0.0
    for j in (1, 2, 3):
        w = 1.0 / np.sum(P[j].astype(np.float64) ** 2)
        wsum += w
        for i in range(4):
            if i == j:
                continue
            f1, f2, f3, _, _ = R.pair_features(P[j], N[j], P[i], N[i])
            for b, coord in enumerate((11 * (f1[0] + np.pi) / (2 * np.pi), 11 * (f2[0] + 1) / 2, 11 * (f3[0] + 1) / 2)):
                want[11 * b + min(10, int(np.floor(coord)))] += w * 100.0 / 3.0
    assert np.allclose(lo[0], want / wsum, atol=1e-12)
    # same_as_surface gives every point a row, and point 0's is the same
    lo_all, _, _ = R.fpfh_interval(P, N, None, 0.1, True, C.TAU)
    assert lo_all.shape == (4, 33) and np.allclose(lo_all[0], lo[0], atol=1e-12)


def test_shot_frame_of_a_hand_made_neighbourhood():
    # three groups, each with every sign combination that keeps the mixed moments zero, so the
    # weighted covariance is diagonal whatever the weights, largest along x, smallest along z:
    # the eight corners of a box, four points at x = +0.3 and four at z = -0.2.  x >= 0 holds for
    # 10 of the 16 neighbours, z >= 0 for 6: x = +e_x, z = -e_z (margins 4 and 4), y = z x x = -e_y
    s = [(a, b) for a in (1, -1) for b in (1, -1)]
    nb = ([(a * 0.5, b * 0.2, c * 0.1) for a, b in s for c in (1, -1)] + [(0.3, a * 0.1, b * 0.05) for a, b in s]
          + [(a * 0.2, b * 0.15, -0.2) for a, b in s])
    P = np.array([(0.0, 0.0, 0.0)] + nb, np.float32)
    rf, (gap, xm, zm) = R.shot_lrf(P, P[0], 1.0)
    assert np.allclose(rf, [1, 0, 0, 0, -1, 0, 0, 0, -1], atol=1e-12)
    assert xm == 4 and zm == 4
    # the eigenvalues are the (1 - d)-weighted means of x^2, y^2 and z^2 over the three groups
    sq = np.array([[0.25, 0.04, 0.01], [0.09, 0.01, 0.0025], [0.04, 0.0225, 0.04]])
    w = np.array([8, 4, 4]) * (1.0 - np.sqrt(sq.sum(1)))
    lam = w @ sq / w.sum()
    assert lam[0] > lam[1] > lam[2]
    assert np.isclose(gap, min(lam[1] - lam[2], lam[0] - lam[1]) / lam[0], rtol=1e-6)
    lam = np.array([8, 4, 4]) @ sq / 16.0
    assert np.isclose(R.shot_lrf(P, P[0], 1.0, dict(lrf_weighted=False))[1][0],
                      min(lam[1] - lam[2], lam[0] - lam[1]) / lam[0], rtol=1e-6)
    assert np.isnan(R.shot_lrf(P[:5], P[0], 1.0)[0]).all()          # four valid neighbours


def test_shot_single_neighbour_lands_in_the_predicted_bins():
    # one voting neighbour (the centre itself is at d = 0, three more points carry no normal) in
    # the identity frame, r = 1: azimuth 100 degrees -> sector 6 (centre 112.5), offset -12.5 / 45,
    # side sector 5; inclination 60 degrees -> upper half, (60 - 45) / 90 = 1/6 to the lower;
    # d = 0.6 -> outer shell, (0.6 - 0.75) / 0.5 = -0.3, so 0.3 to the inner; cos = 0.34 ->
    # (1 + 0.34) * 5 = 6.7 -> bin 7, 0.3 to bin 6
    az, incl, d, cosn = np.radians(100.0), np.radians(60.0), 0.6, 0.34
    p = d * np.array([np.sin(incl) * np.cos(az), np.sin(incl) * np.sin(az), np.cos(incl)])
    P = np.array([[0, 0, 0], p, [0.1, 0.1, 0.1], [-0.2, 0.1, 0.3], [0.3, -0.2, -0.1]])
    N = np.full((5, 3), np.nan)
    N[0] = [0, 0, 1]
    N[1] = [np.sqrt(1 - cosn ** 2), 0, cosn]
    rf = np.eye(3).reshape(9)
    got = R.shot352(P, N, P[0], rf, 1.0).reshape(8, 2, 2, 11)
    a = 12.5 / 45.0
    want = np.zeros((8, 2, 2, 11))
    want[6, 1, 1, 7] = (1 - 0.3) + (1 - 0.3) + (1 - 1.0 / 6.0) + (1 - a)
    want[6, 1, 1, 6] = 0.3          # cosine
    want[6, 0, 1, 7] = 0.3          # radius
    want[6, 1, 0, 7] = 1.0 / 6.0    # elevation
    want[5, 1, 1, 7] = a            # azimuth
    want /= np.sqrt((want ** 2).sum())
    assert (got != 0).sum() == 5
    assert np.allclose(got, want, atol=1e-12)
    # the flat index is ((az * 4 + radial * 2 + elev) * 11 + cos)
    assert R.shot352(P, N, P[0], rf, 1.0)[((6 * 4 + 1 * 2 + 1) * 11) + 7] == got[6, 1, 1, 7]
    # cosine bins wrap modulo 10: cos = 0.86 -> 9.3 -> bin 9, 0.3 to bin 0
    N[1] = [np.sqrt(1 - 0.86 ** 2), 0, 0.86]
    wrap = R.shot352(P, N, P[0], rf, 1.0).reshape(8, 2, 2, 11)
    assert wrap[6, 1, 1, 0] > 0 and wrap[6, 1, 1, 10] == 0
    assert np.isclose(wrap[6, 1, 1, 0] / wrap[6, 0, 1, 9], 1.0, atol=1e-9)   # both 0.3
    assert np.isnan(R.shot352(P[:4], N[:4], P[0], rf, 1.0)).all()            # four neighbours
