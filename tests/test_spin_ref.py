"""The CPU restatement of PCL 1.7 SpinImageEstimation (tests/cpp/spin_ref.cpp) pinned by cases that
follow from DESIGN.md "Spin images: the contract", not by its own output.  No device."""
import math

import numpy as np
import pytest

import pfh_cases as C
import spin_cases as K
import spin_ref as P


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("spin_ref"))


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def one(ref, surface, axis=K.Z, q=K.Q0, **kw):
    """The restatement for the single query q."""
    return P.spin(ref, *surface, *K.points(q), *K.axes(1, axis), K.R, **kw)


def image(row, w=8):
    return np.asarray(row).reshape(w + 1, 2 * w + 1)


def test_one_neighbour_on_the_axis(ref):
    r = one(ref, K.points(K.Q0, K.offset(dz=K.STEP)))
    bs = K.bin_size()
    col = int(math.floor(K.STEP / bs)) + 8
    b = K.STEP / bs - (col - 8)
    want = np.zeros((9, 17))
    want[0, col], want[0, col + 1] = 1.0 - b, b
    assert r.neighbors == 2 and 0.5 < b < 1.0
    assert np.array_equal(image(r.raw[0]), want)
    assert r.sums[0] == 1.0                      # (1 - b) + b is exact for b >= 0.5
    assert np.array_equal(image(r.out[0]), want.astype(np.float32))


def test_one_neighbour_perpendicular_to_the_axis(ref):
    r = one(ref, K.points(K.Q0, K.offset(dx=K.STEP)))
    bs = K.bin_size()
    row = int(math.floor(K.STEP / bs))
    a = K.STEP / bs - row
    want = np.zeros((9, 17))
    want[row, 8], want[row + 1, 8] = 1.0 - a, a   # beta = 0: beta_bin = W, b = 0
    assert np.array_equal(image(r.raw[0]), want)


def test_plane_patch_lies_in_the_middle_column(ref):
    xyz, nrm = C.plane_patch()
    r = P.spin(ref, *xyz, *xyz, *nrm, K.R)
    img = r.out.reshape(-1, 9, 17)
    assert not np.isnan(img).any() and (img[:, :, 8].sum(axis=1) > 0.99).all()
    img[:, :, 8] = 0
    assert not img.any()


def test_inside_the_sphere_outside_the_cylinder_adds_nothing(ref):
    far = K.offset(dz=0.04)                       # d2 < r^2, |beta| >= r / sqrt(2)
    assert 0.04 ** 2 < K.R ** 2 and 0.04 >= K.R / math.sqrt(2.0)
    with_far = one(ref, K.points(K.Q0, K.offset(dz=K.STEP), far))
    without = one(ref, K.points(K.Q0, K.offset(dz=K.STEP)))
    assert with_far.neighbors == 3 and without.neighbors == 2
    assert np.array_equal(bits64(with_far.raw), bits64(without.raw))
    assert np.array_equal(with_far.out, without.out)
    alone = one(ref, K.points(K.Q0, far))         # k = 2, nothing contributes: 0 * inf
    assert alone.sums[0] == 0.0 and np.isnan(alone.out).all() and not alone.raw.any()


def test_nan_axis_is_cosine_one(ref):
    xyz, _ = C.blob(60, K.Q0, 5, side=0.05)       # some neighbours beyond r / sqrt(2)
    q = tuple(float(v[0]) for v in xyz)
    raw, k = K.cos_one_row(xyz, q)
    for axis in ((np.nan, np.nan, np.nan), (0.0, np.nan, 1.0)):
        r = one(ref, xyz, axis=axis, q=q)
        assert r.neighbors == k and r.bad_cos == 0
        assert np.array_equal(bits64(r.raw[0]), bits64(raw))
        img = image(r.raw[0])
        assert img[0].sum() > 0 and not img[1:].any()
        assert np.isfinite(r.out).all()
        want = raw * (1.0 / P.eigen_sum_py(P.column_major(raw, 8)))
        assert np.array_equal(r.out[0], want.astype(np.float32))
    # neighbours at direction_norm >= r / sqrt(2) were dropped: each one kept adds a total weight of 1
    x, y, z = (np.asarray(v, np.float64) for v in xyz)
    dn = np.sqrt((x - q[0]) ** 2 + (y - q[1]) ** 2 + (z - q[2]) ** 2)
    inside = int(((dn > 0) & (dn < K.R / math.sqrt(2.0) - 1e-6)).sum())
    assert inside < k - 1 and abs(raw.sum() - inside) < 1e-9


def test_k0_and_k1_are_zero_rows(ref):
    surface = K.points(K.Q0)
    r = P.spin(ref, *surface, *K.points(K.Q0, K.offset(dx=1.0), (np.nan, 2.0, 3.0)), *K.axes(3), K.R)
    assert r.neighbors == 1 and r.kmax == 1
    assert not r.out.any() and not np.isnan(r.out).any() and not r.sums.any()


def test_all_duplicates_give_a_nan_row(ref):
    r = one(ref, K.points(K.Q0, K.Q0, K.Q0))
    assert r.neighbors == 3 and np.isnan(r.out).all() and r.sums[0] == 0.0
    # 0 * inf on x86-64: the default NaN (sign bit set), and the conversion to float keeps the sign
    assert (r.out.view(np.uint32) == 0xFFC00000).all()


def test_support_angle(ref):
    xyz, nrm, kept = K.support_case()
    r = one(ref, xyz, support_angle_cos=0.5, surface_normals=nrm)
    only = tuple(v[kept] for v in xyz)
    want = one(ref, only)                         # the kept neighbours alone, no support test
    assert r.neighbors == 40 and want.neighbors == int(kept.sum())
    assert np.array_equal(bits64(r.raw), bits64(want.raw)) and np.array_equal(r.out, want.out)
    for i, keep in ((1, False), (2, True), (3, False), (4, True), (5, True), (7, True)):
        two = tuple(v[[0, i]] for v in xyz)
        got = one(ref, two, support_angle_cos=0.5, surface_normals=tuple(v[[0, i]] for v in nrm))
        assert bool(got.raw.any()) == keep, i


def test_bad_cosine_and_too_few(ref):
    surface = K.points(K.Q0, K.offset(dz=K.STEP))
    r = one(ref, surface, axis=(0.0, 0.0, 1.01))
    assert (r.bad_cos, r.first_bad, r.too_few) == (1, 0, 0)
    ok = one(ref, surface, axis=(0.0, 0.0, 1.0 + 1e-6))   # within 1 + 10 FLT_EPSILON: clamped
    assert ok.bad_cos == 0 and np.array_equal(ok.out, one(ref, surface).out)
    r = one(ref, surface, min_pts_neighb=3)
    assert (r.too_few, r.first_few, r.bad_cos) == (1, 0, 0)
    assert one(ref, surface, min_pts_neighb=2).too_few == 0
    # a non-unit surface normal under a support angle breaks the same rule
    nrm = K.f32([0.0, 0.0], [0.0, 0.0], [1.0, 1.01])
    assert one(ref, surface, support_angle_cos=0.5, surface_normals=nrm).bad_cos == 1


@pytest.mark.parametrize("w", [1, 2, 8, 3, 5, 16])
def test_eigen_sum_of_every_tail(ref, w):
    S = P.size(w)
    assert [P.size(v) % 4 for v in (1, 2, 8, 3)] == [2, 3, 1, 0]   # 6, 15, 153, 28
    m = np.random.default_rng(w).uniform(0.0, 1.0, S) * 10.0 ** np.random.default_rng(w + 1).integers(-8, 8, S)
    assert bits64(P.eigen_sum(ref, m)) == bits64(P.eigen_sum_py(m))


def test_eigen_sum_is_not_the_sequential_sum(ref):
    m = np.zeros(153)
    m[0], m[1], m[4] = 1.0, 2.0 ** -53, 2.0 ** -53
    # sequential: 1 + 2^-53 rounds back to 1 twice; four-way: lanes 0 and 1 keep 1 + 2^-53 apart
    m[5] = 2.0 ** -53
    seq, four = P.sequential_sum(m), P.eigen_sum_py(m)
    assert seq == 1.0 and four == 1.0 + 2.0 ** -52 and bits64(seq) != bits64(four)
    assert bits64(P.eigen_sum(ref, m)) == bits64(four)
    for n in (1, 2, 3, 4, 6, 7):
        v = np.arange(1, n + 1) / 3.0
        assert bits64(P.eigen_sum(ref, v)) == bits64(P.eigen_sum_py(v))


def test_reversed_order_changes_raw_bits_on_the_order_case(ref):
    """The teeth of the GPU order test: on its input the accumulation order shows in raw's bits."""
    c = K.order_case()
    fwd = P.spin(ref, *c["xyz"], *c["q"], *c["axes"], K.R)
    rev = P.spin(ref, *c["xyz"], *c["q"], *c["axes"], K.R, reversed_order=True)
    assert fwd.neighbors == 8 * c["k"] and fwd.bad_cos == 0
    differ = (bits64(fwd.raw) != bits64(rev.raw)).any(axis=1)
    assert differ.all(), differ
    assert np.allclose(fwd.raw, rev.raw, rtol=1e-12, atol=1e-15)
    # ... and the summation order shows in sums: the sequential sum differs in bits on some row
    seq = np.array([P.sequential_sum(P.column_major(r, 8)) for r in fwd.raw])
    assert (bits64(seq) != bits64(fwd.sums)).any()
    assert np.array_equal(bits64(fwd.sums), bits64([P.eigen_sum_py(P.column_major(r, 8)) for r in fwd.raw]))
