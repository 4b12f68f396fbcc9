"""The CPU restatement of the shape contexts (tests/cpp/shape_context_ref.cpp) against answers derived
by hand from DESIGN.md "Shape contexts: the contract": the tables, the generator, a lone neighbour's
bin and weight, the frame's branches and the rows that PCL's arithmetic leaves finite.  No GPU."""
import numpy as np
import pytest

import shape_context_cases as K
import shape_context_ref as P
from parity import bits

f = np.float32
X_RND = (1.0, 0.0, 0.5)  # with the normal +z: x = (1, 0, -0), y = (0, 1, 0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("shape_context_ref"))


@pytest.fixture(scope="module")
def tab(ref):
    return P.tables(ref, K.R, K.RMIN)


def one_row(ref, xyz, nrm, rnd=X_RND, q=None, **kw):
    q = K.points(K.Q0) if q is None else q
    return P.shape_context(ref, *xyz, *nrm, *q, K.R, rnd=np.float32(rnd), **kw)


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the tables ----

def test_tables_against_float64(tab):
    radii, theta_div, phi_div, lut = K.tables64()
    assert ulps(tab.radii, radii).max() <= 1 and ulps(tab.theta_div, theta_div).max() <= 1
    assert np.array_equal(tab.phi_div, phi_div.astype(np.float32))
    # the cube root of a product of three float32 differences: the differences of nearby cosines and
    # cubes lose up to ~2^-24 / (their relative size) each, the smallest being the polar caps' 0.04
    rel = np.abs(tab.lut.astype(np.float64) / lut - 1.0).max()
    print("lut: largest relative difference from float64 %.3g" % rel)
    assert rel < 4e-6
    assert tab.radii[0] == f(K.RMIN) and abs(float(tab.radii[15]) - K.R) < 1e-8


def test_table_volume_identity(tab):
    """The bins tile the shell between rmin and R.  PCL's radial integral is r1^3 - r0^3 without the
    third, so the sum of lut^-3 over all 1,980 bins is three times the shell's volume."""
    vol = 12.0 * (tab.lut.astype(np.float64) ** -3).sum()
    want = 4.0 * np.pi * (K.R ** 3 - K.RMIN ** 3)
    assert abs(vol / want - 1.0) < 1e-4


def test_theta_div_ends_at_180(tab):
    """11 * (180.0f / 11.0f) in float32: pinned, since theta = 180 falls through to k = 0 if it is below."""
    assert tab.theta_div[11] == f(11) * (f(180) / f(11))
    print("theta_div[11] = %.9g, phi_div[12] = %.9g, radii[15] = %.9g" % (tab.theta_div[11], tab.phi_div[12], tab.radii[15]))


def test_no_neighbour_lies_above_the_last_radius(tab):
    """For R = 0.08: the largest r of a neighbour is sqrtf of the float below (float)(R R).  Whether
    it exceeds radii[15] decides whether step 6's fall-through (j = 0) can be taken at all."""
    rr = f(K.R * K.R)
    r_max = np.sqrt(np.nextafter(rr, f(0)))
    exists = bool(r_max > tab.radii[15])
    print("r_max = %.9g, radii[15] = %.9g: a neighbour above the last radius %s" %
          (r_max, tab.radii[15], "exists" if exists else "does not exist"))
    assert exists == SC_ABOVE_LAST_RADIUS


SC_ABOVE_LAST_RADIUS = False


# ---- the generator ----

def test_mt19937_known_answer(ref):
    assert P.mt_raw(ref, 5489, 10000)[-1] == 4123659995   # the C++ standard's 10000th output


def test_float_map_redraws_when_the_cast_rounds_to_one(ref):
    top = 0xffffffff
    raw = np.array([0, 1 << 31, top - 128, top - 127, top, 12345], np.uint32)
    # (float)u32 rounds to 2^32 from 2^32 - 128 up (ties to even): those two are drawn again
    want = np.float32([0.0, 0.5, f(top - 128) * f(2.0 ** -32), f(12345) * f(2.0 ** -32)])
    assert f(top - 128) < f(2.0 ** 32) and f(top - 127) == f(2.0 ** 32)
    assert np.array_equal(P.map01(ref, raw), want) and want[2] < 1.0


def test_stream_skip_composes_and_matches_the_library(ref):
    from pcl_feature_extraction_amd import uniform01_stream
    a = P.uniform01(ref, 12345, 4000)
    assert np.array_equal(P.uniform01(ref, 12345, 1000, skip=3000), a[3000:])
    raw = P.mt_raw(ref, 12345, 4000)
    assert np.array_equal(a, (raw.astype(np.float32) * f(2.0 ** -32)))   # no redraw this early
    assert np.array_equal(uniform01_stream(12345, 4000), a)
    assert np.array_equal(uniform01_stream(12345, 7, skip=3993), a[3993:])
    assert np.array_equal(uniform01_stream(777, 64), P.uniform01(ref, 777, 64))
    assert a.min() >= 0.0 and a.max() < 1.0


def test_usc_360_is_the_same_in_float_and_double():
    """(M) `360.0 - phi` in double, rounded to float, equals the float subtraction for every float phi
    the arctangent gives: the difference is exact in double unless phi < 2^-20, where both are 360."""
    rng = np.random.default_rng(5)
    phi = np.concatenate([rng.uniform(0, 180.001, 200000), 10.0 ** rng.uniform(-40, 0, 50000)]).astype(np.float32)
    assert np.array_equal((360.0 - phi.astype(np.float64)).astype(np.float32), f(360) - phi)


# ---- a lone neighbour ----

def test_one_neighbour_one_bin(ref, tab):
    xyz, nrm = K.lone_neighbour()
    got = one_row(ref, xyz, nrm)
    # r = sqrt(3) / 64 = 0.02706 in (radii[7], radii[8]], theta = acos(1 / sqrt 3) = 54.7 in (49.1, 65.5],
    # phi = 45 in (30, 60]
    assert K.bin_of(K.offset(K.STEP, K.STEP, K.STEP), K.Q0, (1, 0, 0), (0, 0, 1), tab) == (1, 3, 7)
    row = got.desc[0]
    assert np.flatnonzero(row).tolist() == [K.flat(1, 3, 7)] == [217]
    assert row[217] == tab.lut[3, 7]          # its own density is 1 (the query is 0.027 > rho away)
    assert np.array_equal(got.rf[0], f([1, 0, -0.0, 0, 1, 0, 0, 0, 1]))
    assert (got.neighbors, got.kmax, got.draws, got.skipped_close, got.support) == (2, 2, 1, 1, 2)
    # the other half turn: x = (-1, 0, 0) gives phi = 360 - 135 = 225 in (210, 240]
    row = one_row(ref, xyz, nrm, rnd=(-1.0, 0.0, 0.5)).desc[0]
    assert np.flatnonzero(row).tolist() == [K.flat(7, 3, 7)]


def test_density_divides_the_weight(ref, tab):
    """Two neighbours 2^-13 apart share a bin and a density of 2: lut / 2 + lut / 2."""
    xyz = K.points(K.Q0, K.offset(K.STEP, K.STEP, K.STEP), K.offset(K.STEP, K.STEP, K.STEP + 2.0 ** -13))
    got = one_row(ref, xyz, K.vectors(3, (0, 0, 1)))
    row = got.desc[0]
    assert np.flatnonzero(row).tolist() == [217] and row[217] == f(0.5) * tab.lut[3, 7] + f(0.5) * tab.lut[3, 7]


@pytest.mark.parametrize("normal, rnd, x, y", [
    ((0, 0, 1), (3, 4, 9), (0.6, 0.8, -0.0), (-0.8, 0.6, 0)),     # n.z != 0: x.z follows
    ((0, 1, 0), (3, 9, 4), (0.6, -0.0, 0.8), (0.8, 0, -0.6)),     # n.z == 0, n.y != 0: x.y follows
    ((1, 0, 0), (9, 3, 4), (-0.0, 0.6, 0.8), (0, -0.8, 0.6)),     # only n.x != 0: x.x follows
    ((0, 0, 0), (3, 0, 4), (0.6, 0, 0.8), (0, 0, 0)),             # a zero normal: no branch taken
])
def test_orthogonalisation_branches(ref, normal, rnd, x, y):
    xyz, nrm = K.lone_neighbour(normal=normal)
    rf = one_row(ref, xyz, nrm, rnd=rnd).rf[0]
    assert np.allclose(rf[:3], x, atol=1e-7) and np.allclose(rf[3:6], y, atol=1e-7)
    assert np.array_equal(rf[6:], f(normal))
    if any(normal):
        assert abs(np.dot(rf[:3], rf[6:])) < 1e-7


def test_nan_normal_keeps_the_row_finite(ref, tab):
    """x and y are NaN; phi is NaN (l = 0) and the cosine's clamp turns NaN into -1 (theta = 180)."""
    xyz, nrm = K.lone_neighbour(normal=(np.nan, 0.0, 1.0))
    got = one_row(ref, xyz, nrm)
    assert (bits(got.rf[0, :7]) == K.NAN_BITS).all() and np.array_equal(got.rf[0, 7:], f([0, 1]))
    row = got.desc[0]
    k180 = K.first_division(f(np.arccos(f(-1))) * f(57.29578), tab.theta_div)
    assert np.isfinite(row).all() and np.flatnonzero(row).tolist() == [K.flat(0, k180, 7)]
    assert row[K.flat(0, k180, 7)] == tab.lut[k180, 7]


def test_neighbours_on_the_normal_axis(ref, tab):
    """The projection is the zero vector: its normalisation is NaN, phi is NaN, l = 0.  theta is
    exactly 0 above the query and 180 (as the float arccosine of -1 times the float factor) below."""
    k180 = K.first_division(f(np.arccos(f(-1))) * f(57.29578), tab.theta_div)
    for dz, k in ((2 * K.STEP, 0), (-2 * K.STEP, k180)):   # (2^-5 > rho: the neighbour's density is 1)
        xyz, nrm = K.lone_neighbour(step=(0.0, 0.0, dz))
        row = one_row(ref, xyz, nrm).desc[0]
        j = K.first_division(2 * K.STEP, tab.radii)
        assert np.flatnonzero(row).tolist() == [K.flat(0, k, j)] and row[K.flat(0, k, j)] == tab.lut[k, j]
    print("theta = 180 falls into elevation bin %d" % k180)


def test_close_point_skip_on_either_side_of_epsilon(ref):
    """equal(d2, 0) = |d2| < FLT_EPSILON = 2^-23.  One axis offset 2^-12: d2 = 2^-24, skipped.  Two: d2 =
    2^-23 exactly, kept."""
    e = 2.0 ** -12
    xyz = K.points(K.Q0, K.offset(e), K.offset(0.0, e, e))
    got = one_row(ref, xyz, K.vectors(3, (0, 0, 1)))
    assert (got.neighbors, got.skipped_close) == (3, 2)
    row = got.desc[0]
    assert len(np.flatnonzero(row)) == 1 and row.sum() > 0


def test_special_rows(ref):
    xyz, nrm = K.lone_neighbour()
    q = K.points((9.0e3, 9.0e3, 9.0e3), (np.nan, 2.0, 3.0), K.Q0)
    got = P.shape_context(ref, *xyz, *nrm, *q, K.R, rnd=np.float32([1, 0, 0.5] + [7] * 6))
    # no neighbour and a non-finite query: NaN, no frame, no draw; the third row takes the first draw
    assert (bits(got.desc[:2]) == K.NAN_BITS).all() and not got.rf[:2].any() and got.draws == 1
    assert np.array_equal(got.rf[2], f([1, 0, -0.0, 0, 1, 0, 0, 0, 1]))
    frames = np.float32([[1, 0, 0, 0, 1, 0, 0, 0, 1]] * 3)
    u = P.usc(ref, *xyz, *q, frames, K.R)
    assert not u.desc[0].any() and np.array_equal(u.rf[0], frames[0])      # USC, k = 0: a zero row in its frame
    assert (bits(u.desc[1]) == K.NAN_BITS).all() and not u.rf[1].any()
    assert np.array_equal(bits(u.desc[2]), bits(got.desc[2]))             # the same frame: the same row
    for bad in (0, 3, 6):
        fr = frames.copy()
        fr[2, bad] = np.nan
        u = P.usc(ref, *xyz, *q, fr, K.R)
        assert (bits(u.desc[2]) == K.NAN_BITS).all() and not u.rf[2].any()


def test_duplicates(ref):
    """Copies of the query are skipped; copies of a neighbour count in each other's density."""
    p = K.offset(K.STEP, K.STEP, K.STEP)
    xyz = K.points(K.Q0, K.Q0, p, p, p)
    got = one_row(ref, xyz, K.vectors(5, (0, 0, 1)))
    row = got.desc[0]
    assert got.skipped_close == 2 and np.flatnonzero(row).tolist() == [217]
    third = f(1) / f(3)
    t = P.tables(ref, K.R, K.RMIN).lut[3, 7]
    assert row[217] == (third * t + third * t) + third * t


def test_the_order_decides_bits(ref):
    c = K.order_case()
    a = P.shape_context(ref, *c["xyz"], *c["normals"], *c["q"], K.R)
    b = P.shape_context(ref, *c["xyz"], *c["normals"], *c["q"], K.R, reversed_order=True)
    assert a.kmax == c["k"] and np.array_equal(a.rf, b.rf)
    assert (bits(a.desc) != bits(b.desc)).any() and np.allclose(a.desc, b.desc, rtol=1e-5)


def test_rim_density_sees_points_outside_every_query_ball(ref, tab):
    c = K.rim_case()
    got = one_row(ref, c["xyz"], c["normals"], q=c["q"])
    row = got.desc[0]
    (b,) = np.flatnonzero(row)
    assert (got.neighbors, got.support) == (2, 2)
    assert row[b] == (f(1) / f(c["density"])) * tab.lut[(b % 165) // 15, b % 15]
