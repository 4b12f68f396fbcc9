"""Closed forms that pin the CPU restatement of the NARF descriptor (tests/cpp/narf_desc_ref.cpp, the
truth the kernel is tested against) on synthetic range images small enough to reason about, and of
Tools::getIndices.  The scenes are in narf_desc_cases.py.  Every bound is derived in the test from
the float32 format and the sizes involved, and the figure met is printed before it is asserted."""
import numpy as np
import pytest

import narf_desc_cases as K
import narf_desc_ref as P

EPS = 2.0 ** -24  # half an ulp of 1 in float32
SUPPORT, MAX_DIST = 0.2, 0.1
BEAM_W = np.array([2.0 * 2.0 / 3.0 - 2.0 / 27.0 * j for j in range(10)])  # wf j + wo


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("narf_desc_ref"))


def one(ref, depth, cam, pix, rotinv=False, support=SUPPORT):
    return P.on_image(ref, K.depth_image(depth, cam), [pix], support, rotinv, cam, debug=True)


def beam_sums(desc):
    """tan (pi d[k]) max_dist: the weighted sum s of the contract's step 6."""
    return np.tan(np.pi * np.asarray(desc, np.float64)) * MAX_DIST


def model_sums(blur):
    """Step 6 on a blurred patch: the sample cells with the contract's float32 steps (a beam along a
    cell border falls to the side its float32 angle sends it), the sums in float64."""
    f = np.float32
    step = f(f(360.0) * f(0.017453293)) / f(36)
    cell = f(SUPPORT) / f(20.0)
    cf, co, bpf = f(1.0) / cell, f(0.5) * (f(SUPPORT) - cell), (f(0.5) * f(SUPPORT) - f(0.5) * cell) / f(10)
    out = []
    for k in range(36):
        angle = f(k) * step
        fx, fy = f(np.sin(np.float64(angle))) * bpf, -f(np.cos(np.float64(angle))) * bpf
        b = [blur[int(np.rint(cf * (fy * f(j) + co))), int(np.rint(cf * (fx * f(j) + co)))] for j in range(11)]
        out.append(sum(BEAM_W[j] * (b[j + 1] - b[j]) for j in range(10)))
    return np.array(out)


def box_blur(patch10):
    """Step 5 in float64: every patch cell twice in each axis, then the mean over the 3 x 3 window
    clipped at the border."""
    raw = np.repeat(np.repeat(np.asarray(patch10, np.float64), 2, 0), 2, 1)
    return np.array([[raw[max(0, y - 1):y + 2, max(0, x - 1):x + 2].mean() for x in range(20)] for y in range(20)])


# ---- a fronto-parallel wall ------------------------------------------------------------------

def test_wall_has_the_identity_pose_a_zero_patch_and_no_rotation(ref):
    """Every ring point has z = 2 exactly, so the z row and column of the covariance are exact zeros:
    the normal is (0, 0, 1) after the sign rule (away from the sensor), the rows are the world axes,
    the translation -(0, 0, 2); every patch cell is seen and 0, the descriptor 36 zeros.  All 36
    scores are then 0.5: with rotation invariance there is no row."""
    r = one(ref, 2.0, K.T, K.T_CENTRE)
    assert r.stats == dict(rows=1, invalid_pixels=0, pose_failed=0, fallback_normals=0, ring_max=r.stats["ring_max"],
                           background_cells=0)
    assert np.array_equal(r.pose[0].reshape(3, 4), np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -2]], np.float32))
    assert np.array_equal(r.patch[0], np.zeros((10, 10), np.float32))
    assert np.array_equal(r.desc, np.zeros((1, 36), np.float32)) and r.keypoint.tolist() == [0]
    # the patch spans +-5 pixels (0.1 m at 2 m with f = 100): ring 6 is the first past it for both walks
    assert 6 <= r.stats["ring_max"] <= 8
    inv = one(ref, 2.0, K.T, K.T_CENTRE, rotinv=True)
    assert len(inv.desc) == 0 and inv.stats["rows"] == 0 and inv.stats["pose_failed"] == 0


def test_tilted_wall_stays_within_the_rounding_of_its_pose(ref):
    """The plane n0 . q = c0 tilted by 0.3 rad.  With r the pose's third row and t its translation, a
    point q of the plane has patch height r . q + t = (+-c0 + t) + dr . q, dr = r -+ n0.  The
    image's points are the plane's rounded to float32 (|r|_1 EPS |q| more) and the height is three
    products and three sums at magnitude S = |r| . |q| + |t| (6 EPS S more).  A cell's value is a
    combination of three such heights with coefficients of absolute sum <= 1.04 (u, v >= -0.01, u + v
    <= 1.01).  The blur averages, the beam weights add to 10 and each multiplies a difference of two
    values, atan (s / max_dist) / pi <= s / (pi max_dist): |d| <= 20 bound / (pi max_dist)."""
    a = 0.3
    n0 = np.array([np.sin(a), 0.0, np.cos(a)])
    c0 = n0[2] * 2.0
    ri = K.depth_image(K.plane_depth(n0, 2.0), K.T)
    r = P.on_image(ref, ri, [K.T_CENTRE], SUPPORT, False, K.T, debug=True)
    assert r.stats["rows"] == 1 and r.stats["fallback_normals"] == 0 and np.isfinite(r.patch).all()
    pose = r.pose[0].reshape(3, 4).astype(np.float64)
    row, t = pose[2, :3], pose[2, 3]
    sgn = np.sign(row @ n0)
    qmax = np.abs(ri[..., :3].astype(np.float64)).sum(-1).max()  # |q|_1 >= |q|_2 >= |q|_inf
    S = np.abs(row).max() * qmax + abs(t)
    e = abs(sgn * c0 + t) + np.linalg.norm(row - sgn * n0) * qmax + np.abs(row).sum() * EPS * qmax + 6 * EPS * S
    bound = 1.04 * e
    print("tilted wall: max |patch| %.3g, bound %.3g; max |d| %.3g" % (np.abs(r.patch).max(), bound, np.abs(r.desc).max()))
    assert sgn == 1.0  # (away from the sensor)
    assert bound < 64 * EPS * qmax  # the pose itself is within a few ulp of the coordinates of the exact one
    assert np.abs(r.patch).max() <= bound
    assert np.abs(r.desc).max() <= 20 * bound / (np.pi * MAX_DIST)


# ---- a step of height delta ------------------------------------------------------------------

def test_step_across_the_patch_gives_delta_times_the_beam_weight_at_the_crossing(ref):
    """The strip |x| < 0.04 at z = 2 between two walls at z = 2 + delta (even in x and y: the normal
    stays the optical axis; a one-sided step would tilt the pose and with it every cell).  Patch
    columns 3..6 (|x| <= 0.03) are near, the others far; in the 20 x 20 image columns 6..13 are near, and
    the 3-cell blur gives, as fractions of delta above the near level, 0 in columns 7..12, 1/3 in 6 and
    13, 2/3 in 5 and 14, 1 beyond.  A beam's sum is delta times sum_j w_j (g[j + 1] - g[j]) with g
    that fraction at its j-th sample: the weight w_j = 4/3 - 2 j / 27 at the crossing, spread over the
    three blurred columns.  Beams within 15 degrees of the strip's axis never leave columns 7..12: 0.
    Opposite beams are equal here (the scene is even).
    Tolerance, as a fraction of delta: a blurred value is norm (BR + TL - BL - TR) of integral-image
    entries up to 400 V (V the largest |patch value|); the entries' own errors cancel outside the
    window, leaving 9 cells' three roundings each of 2 EPS 400 V, times norm = 1/9, plus three
    roundings of the combination: e_b = (3 + 3 / 9) 2 EPS 400 V; a patch value carries three roundings at
    magnitude 2 + delta from the transform: e_p = 3 EPS 2.03; s = -w_0 b_0 + sum (w_{j-1} - w_j) b_j +
    w_9 b_10 has coefficients of absolute sum 8/3."""
    delta = 0.03
    r = one(ref, K.groove_depth(0.04, delta), K.Q, K.Q_CENTRE)
    assert r.stats["rows"] == 1 and r.stats["background_cells"] == 0 and np.isfinite(r.patch).all()
    pose = r.pose[0].reshape(3, 4)
    assert np.abs(pose[:, :3] - np.eye(3)).max() < 16 * EPS  # upright, to rounding
    patch = r.patch[0].astype(np.float64)
    near = patch[:, 3:7]
    assert np.ptp(near) < 8 * EPS * 2 and np.abs(patch[:, [0, 1, 2, 7, 8, 9]] - near.mean() - delta).max() < 8 * EPS * 2
    g = np.ones((10, 10))
    g[:, 3:7] = 0.0
    want = model_sums(box_blur(g))
    got = beam_sums(r.desc[0]) / delta
    V = np.abs(patch).max()
    tol = (8.0 / 3.0) * ((3 + 3 / 9) * 2 * EPS * 400 * V + 3 * EPS * 2.03) / delta
    print("step: max |s / delta - model| %.3g, tolerance %.3g" % (np.abs(got - want).max(), tol))
    assert np.abs(got - want).max() <= tol
    quiet = [0, 1, 17, 18, 19, 35]
    assert np.array_equal(r.desc[0][quiet], np.zeros(6, np.float32)) and np.all(want[quiet] == 0)
    # the beam along +x samples columns 10, 10, 11, 12, 13, 14, 15, ...: thirds of delta at j = 3, 4 and 5
    assert want[9] == pytest.approx((BEAM_W[3] + BEAM_W[4] + BEAM_W[5]) / 3)
    assert np.all(got[2:17] > 0.2) and np.allclose(got[:18], got[18:], atol=2 * tol)


def test_opposite_beams_across_a_step_through_the_centre_have_opposite_signs(ref):
    """Steps 5 and 6 alone on a patch that is -delta / 2 left of the centre and +delta / 2 right of it
    (through the whole pipeline such a scene tilts the pose): the beams to the right climb, those to
    the left descend, the two along the step stay; every sum is the model's."""
    delta = 0.03
    patch = np.full((10, 10), -delta / 2, np.float32)
    patch[:, 5:] = delta / 2
    blur, d = P.patch_descriptor(ref, patch, SUPPORT)
    assert np.abs(blur - box_blur(patch)).max() <= (3 + 3 / 9) * 2 * EPS * 400 * delta / 2
    s = beam_sums(d)
    assert np.abs(s - model_sums(box_blur(patch))).max() <= (8.0 / 3.0) * (3 + 3 / 9) * 2 * EPS * 400 * delta / 2
    assert np.all(s[1:18] > 0) and np.all(s[19:36] < 0) and np.all(s[1:18] * s[19:36] < 0)
    # along +x: columns 10, 10, 11 hold delta / 6, delta / 6, delta / 2: one rise of delta / 3 at j = 1
    assert s[9] == pytest.approx(delta * BEAM_W[1] / 3, rel=1e-4)


# ---- a quarter turn of the scene -------------------------------------------------------------

def test_quarter_turn_of_the_scene_shifts_the_descriptor_by_nine_entries(ref):
    """A relief that is even about the keypoint (the normal stays the optical axis) turned by 90 degrees
    about it: np.rot90 of the depth map, since the pixels are square and the centre is a pixel.  The
    world point at patch (x, y) moves to (-y, x) ... so the beam at angle t sees what the beam at t -
    90 degrees saw: d'[(k + 9) % 36] = d[k], and the invariant rows' rotations move by +90 degrees.
    The relief's evenness makes the descriptor 18-periodic, so this test cannot tell +90 from -90 degrees:
    the next test, with turns that are no multiple of 90 degrees, pins the direction.  Even the quarter
    turn is not exact to rounding: the
    20 x 20 blurred image has its centre between cells, every beam starts in cell (10, 10) (9.5 rounds
    to even), and the turn maps that cell onto (9, 10); the other samples may likewise fall one cell
    to the side in either axis.  So each sample moves by at most 2 G, G the largest difference of
    adjacent blurred cells, and with the coefficients of s (absolute sum 8/3) |d' - d| <= (8/3) 2 G
    / (pi max_dist).  That bound exceeds the descriptor's amplitude here, so it decides nothing: what
    decides is that the error is a quarter of any other shift's.  DESIGN.md records the figures met."""
    z0 = K.relief_depth(K.even_relief)
    a, ai = one(ref, z0, K.Q, K.Q_CENTRE), one(ref, z0, K.Q, K.Q_CENTRE, rotinv=True)
    assert np.abs(a.pose[0].reshape(3, 4)[:, :3] - np.eye(3)).max() < 1e-5
    blur = a.blur[0].astype(np.float64)
    G = max(np.abs(np.diff(blur, axis=0)).max(), np.abs(np.diff(blur, axis=1)).max())
    bound = (8.0 / 3.0) * 2 * G / (np.pi * MAX_DIST)
    assert len(ai.rot) >= 2
    for q, shift in ((1, 9), (3, 27)):  # rot90 turns the image by -90 degrees for q = 1 (y points down)
        zq = np.rot90(z0, q)
        b, bi = one(ref, zq, K.Q, K.Q_CENTRE), one(ref, zq, K.Q, K.Q_CENTRE, rotinv=True)
        err = np.abs(np.roll(a.desc[0], shift) - b.desc[0]).max()
        by_shift = np.array([np.abs(np.roll(a.desc[0], m) - b.desc[0]).max() for m in range(36)])
        print("quarter turn %d: max |d' - d| %.3g (bound %.3g, amplitude %.3g, the best other shift: %.3g)"
              % (q, err, bound, np.abs(a.desc).max(), np.delete(by_shift, [9, 27]).min()))
        assert err <= bound
        # (the scene is even, so 9 and 27 are the same shift) no other shift comes near
        assert set(np.argsort(by_shift)[:2].tolist()) == {9, 27} and 4 * err < np.delete(by_shift, [9, 27]).min()
        # the rows' rotations move by the same angle (as a set: the even scene's two rotations score
        # within rounding of each other, so their order is not the scene's)
        turn = np.float32(shift * 10.0 * 0.017453293)
        moved = np.sort(np.arctan2(np.sin(ai.rot + turn), np.cos(ai.rot + turn)))
        assert len(bi.rot) == len(ai.rot) and np.abs(np.sort(bi.rot) - moved).max() < 1e-5
        assert max(np.abs(row - ai.desc).max(axis=1).min() for row in bi.desc) <= bound


def circular(a, b):
    return np.abs(np.arctan2(np.sin(a - b), np.cos(a - b)))


@pytest.mark.parametrize("m", [1, 2, 4, 7, 32])
def test_turn_by_m_steps_shifts_the_descriptor_by_plus_m_entries(ref, m):
    """The direction of the shift.  The even relief turned by +m 10 degrees about the optical axis (x
    towards y; the analytic height function is turned, not the image): a feature the beam at angle t
    saw (direction (sin t, -cos t) in the patch, whose axes are the world's here) is now seen by the beam
    at t + m 10 degrees: d'[(k + m) % 36] = d[k], and every invariant row's rotation moves by +m 10
    degrees.  The relief is even, so the descriptor has period 18 and a shift is known modulo 18; for
    m no multiple of 9, +m, -m and m +- 9 are different shifts modulo 18, so the sign of the beam
    direction and of rho is observed (m = 32 is -4).  These turns do not map the patch grid onto itself,
    so the agreement is to the 10 x 10 patch's resolution: the assertion is that +m is the best of the 18
    shifts, by the margin met (the best shift's error is at most 0.74 of the second best's,
    at m = 1), and that the mirrored shift -m is worse than the second best."""
    a, ai = one(ref, K.relief_depth(K.even_relief), K.Q, K.Q_CENTRE), \
        one(ref, K.relief_depth(K.even_relief), K.Q, K.Q_CENTRE, rotinv=True)
    phi = np.radians(10.0 * m)
    z = K.relief_depth(K.turned(K.even_relief, phi))
    b, bi = one(ref, z, K.Q, K.Q_CENTRE), one(ref, z, K.Q, K.Q_CENTRE, rotinv=True)
    assert np.abs(b.pose[0].reshape(3, 4)[:, :3] - np.eye(3)).max() < 1e-5  # still upright
    by_shift = np.array([np.abs(np.roll(a.desc[0], k) - b.desc[0]).max() for k in range(18)])
    order = np.argsort(by_shift)
    print("turn by %d steps: shifts by error %s: %s (amplitude %.3g; shift -m: %.3g)"
          % (m, order[:3].tolist(), by_shift[order[:3]].round(5).tolist(), np.abs(a.desc).max(), by_shift[(-m) % 18]))
    assert order[0] == m % 18
    assert by_shift[order[0]] <= 0.8 * by_shift[order[1]]
    assert by_shift[(-m) % 18] > by_shift[order[1]]
    # the rotations: each of the original's, moved by +phi, is one of the turned scene's
    assert len(bi.rot) == len(ai.rot) >= 2
    for r0 in ai.rot:
        assert circular(bi.rot, r0 + phi).min() < 1e-4
        assert circular(bi.rot, r0 - phi).min() > 0.1  # (not by -phi)
    # ... and the rows themselves do not move: the descriptor at rho + phi of the turned scene is the
    # one at rho of the original (were rho to run against the beam index, they would differ by 2 m
    # entries either way); met: at most 0.0037 against 0.011 and more
    unmoved = max(np.abs(row - ai.desc).max(axis=1).min() for row in bi.desc)
    for k in (2 * m, -2 * m):
        rolled = min(np.abs(row - np.roll(ai.desc, k % 36, axis=1)).max(axis=1).min() for row in bi.desc)
        assert unmoved <= 0.5 * rolled, (unmoved, rolled)


# ---- background cells ------------------------------------------------------------------------

def test_square_in_front_of_a_far_wall_marks_background_and_alone_does_not(ref):
    """A 9 cm square at 2 m: patch cells 3..6 in both axes are seen and 0.  With a wall 1 m behind
    (more than max_dist), the unseen cells beside a seen one look past the square's edge at something
    1 m further: background, +inf, and so are their unseen neighbours: the 8 x 8 block but the 16 seen
    cells; the outermost ring stays -inf.  With nothing behind, the range difference is -inf and every
    unseen cell stays -inf."""
    far = one(ref, K.square_depth(3.0), K.Q, K.Q_CENTRE)
    want = np.full((10, 10), -np.inf, np.float32)
    want[1:9, 1:9] = np.inf
    want[3:7, 3:7] = 0.0
    assert np.array_equal(far.patch[0], want) and far.stats["background_cells"] == 48 and far.stats["rows"] == 1
    alone = one(ref, K.square_depth(np.nan), K.Q, K.Q_CENTRE)
    want[want == np.inf] = -np.inf
    assert np.array_equal(alone.patch[0], want) and alone.stats["background_cells"] == 0 and alone.stats["rows"] == 1
    # either infinity reads as max_dist in the blur, so the two descriptors are the same
    assert np.array_equal(far.desc, alone.desc) and np.all(far.desc[0] > 0)


# ---- row counts ------------------------------------------------------------------------------

def test_fallback_failure_and_invalid_entries_give_the_contracts_row_counts(ref):
    """Camera T at 2 m: a pixel is 2 cm.  With support 0.05 only the four direct neighbours (2 cm, the
    diagonals are 2.83 cm) lie within max_dist = 2.5 cm: 4 samples <= 10, the fallback normal from the 5 x
    5 window, one row.  A pixel alone in an empty 7 x 7 window has neither: no row, pose_failed.  A
    pixel without a range, a negative index and one beyond the image: no row, invalid_pixels."""
    depth = np.full((K.T["height"], K.T["width"]), 2.0)
    depth[:9, :9] = np.nan
    depth[4, 4] = 2.0
    ri = K.depth_image(depth, K.T)
    w, npx = K.T["width"], K.T["width"] * K.T["height"]
    pix = [K.T_CENTRE, 4 * w + 4, 1 * w + 1, -1, npx, npx - 1]
    r = P.on_image(ref, ri, pix, 0.05, False, K.T)
    assert r.keypoint.tolist() == [0, 5]  # the centre and the corner pixel (its window is cut by the image)
    assert r.stats == dict(rows=2, invalid_pixels=3, pose_failed=1, fallback_normals=2,
                           ring_max=r.stats["ring_max"], background_cells=r.stats["background_cells"])
    assert np.array_equal(r.pose[0].reshape(3, 4)[2, :3], np.array([0, 0, -1], np.float32))  # towards the sensor
    # with the usual support the same entries: the two rows without the fallback
    r = P.on_image(ref, ri, pix, SUPPORT, False, K.T)
    assert r.keypoint.tolist() == [0, 5] and r.stats["fallback_normals"] == 0 and r.stats["pose_failed"] == 1
    assert np.array_equal(r.pose[0].reshape(3, 4)[2, :3], np.array([0, 0, 1], np.float32))  # away from it


# ---- several rotations -----------------------------------------------------------------------

def test_x_ridge_gives_four_rotations_a_quarter_turn_apart(ref):
    r = one(ref, K.relief_depth(K.x_ridge), K.Q, K.Q_CENTRE, rotinv=True)
    assert len(r.desc) == 4 and r.keypoint.tolist() == [0, 0, 0, 0] and r.stats["rows"] == 4
    deg = np.sort(np.degrees(r.rot.astype(np.float64)))
    assert np.allclose(deg, [-180, -90, 0, 90], atol=1e-3)
    # each row is the descriptor seen from its own rotation: the four agree to the patch's resolution
    assert np.abs(r.desc - r.desc[0]).max() < 0.1 * np.abs(r.desc[0]).max()
    # pose_row = Rz (-rho) pose: the third rows agree, the first turn
    p = r.pose.reshape(4, 3, 4)
    assert np.array_equal(p[:, 2], np.repeat(p[:1, 2], 4, 0))
    for k in range(4):
        c, s = np.cos(-r.rot[k].astype(np.float64)), np.sin(-r.rot[k].astype(np.float64))
        rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        base = np.linalg.inv(rz) @ p[k].astype(np.float64)
        assert np.abs(base - np.linalg.inv(np.array([[np.cos(-r.rot[0]), -np.sin(-r.rot[0]), 0],
                                                      [np.sin(-r.rot[0]), np.cos(-r.rot[0]), 0], [0, 0, 1]])) @ p[0]).max() < 1e-5


def test_rotation_ties_go_to_the_higher_step_and_equal_scores_drop_everything(ref):
    """Two equal peaks half a turn apart: steps 9 and 27 tie exactly (each sees its own peak with
    weight 1 and the other with weight 0); step 27 (+90 degrees) is taken first, then step 9.  One peak:
    one rotation, its own angle.  A flat descriptor: all scores 0.5, nothing survives the threshold."""
    step = np.float32(360.0 * 0.017453293) / np.float32(36)
    d0 = np.zeros(36, np.float32)
    d0[9] = d0[27] = 0.1
    rot, score = P.rotations(ref, d0)
    assert score[9] == score[27] == score.max()
    assert rot.tolist() == [np.float32(27) * step - np.float32(np.pi), np.float32(9) * step - np.float32(np.pi)]
    d0[:] = 0
    d0[20] = 0.2
    rot, score = P.rotations(ref, d0)
    assert rot.tolist() == [np.float32(20) * step - np.float32(np.pi)] and score.argmax() == 20
    assert score[20] == pytest.approx(0.5 + 0.2 / 36, rel=1e-6)
    rot, score = P.rotations(ref, np.zeros(36, np.float32))
    assert len(rot) == 0 and np.all(score == 0.5)


# ---- point indices ---------------------------------------------------------------------------

def test_point_indices_are_those_of_get_indices(ref):
    x = np.array([0.0, 1.0, 1.0, 2.0, 1.0, np.nan, 3.0], np.float32)
    y = np.array([0.0, 1.0, 1.0, 2.0, 1.0, 0.0, 3.0], np.float32)
    z = np.array([0.0, 1.0, 1.0, 2.0, 1.0, 0.0, 3.0], np.float32)
    tol = np.float32(1e-4)
    near, past = np.float32(2.0) + np.float32(0.99e-4), np.float32(2.0) + np.float32(1.01e-4)
    assert abs(near - np.float32(2.0)) < tol < abs(past - np.float32(2.0))
    kx = np.array([3.0, 1.0, 0.5, near, past, 2.0, 2.0, np.nan, 0.0], np.float32)
    ky = np.array([3.0, 1.0, 0.5, 2.0, 2.0, near, 2.0, 0.0, 0.0], np.float32)
    kz = np.array([3.0, 1.0, 0.5, 2.0, 2.0, 2.0, past, 0.0, np.nan], np.float32)
    # keypoint order, cloud indices ascending within one; the duplicates all found; NaN matches nothing
    assert P.point_indices(ref, x, y, z, kx, ky, kz).tolist() == [6, 1, 2, 4, 3, 3]
    assert P.point_indices(ref, x, y, z, kx[:0], ky[:0], kz[:0]).tolist() == []
    assert P.point_indices(ref, x[:0], y[:0], z[:0], kx, ky, kz).tolist() == []
    assert P.point_indices(ref, x, y, z, kx, ky, kz, tol=1.5).tolist()[:3] == [3, 6, 0]
