"""The CPU restatement of CVFH (tests/cpp/cvfh_ref.cpp) pinned on closed forms, so that the GPU tests
(tests/test_gpu_cvfh.py) compare the kernels with something that is itself checked: a flat patch whose
bins follow from the geometry, the clusters against an independent numpy union-find, the bisected
angle threshold against acos itself, and the rows as sequential float sums of their counts."""
import numpy as np
import pytest

import cvfh_cases as K
import cvfh_ref as R
import oracle_lib as O

F = np.float32
BLOCKS = ((0, 45), (45, 90), (90, 135), (135, 180), (180, 308))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("cvfh_ref"))


@pytest.fixture(scope="module")
def roof():
    xyz = K.roof()
    return xyz + tuple(O.normals(*xyz, 0.02))


def flat_patch(m=20):
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    xyz = K.f32(0.3 + 0.004 * i.ravel(), 0.2 + 0.004 * j.ravel(), np.ones(m * m))
    return xyz + K.flat_normals(m * m)


def test_flat_patch(ref):
    s = flat_patch()
    n = len(s[0])
    r = R.cvfh(ref, O.normals, *s)
    assert r.stats == dict(cvfh_filtered=n, cvfh_clusters=1, cvfh_edges=r.stats["cvfh_edges"],
                           cvfh_cc_rounds=r.stats["cvfh_cc_rounds"], cvfh_rows=1)
    assert set(r.labels) == {0} and r.rows.shape == (1, 308)
    c = r.counts[0]
    # every point's direction from the centroid lies in the plane: f3 = 0, the middle bin
    assert c[90 + 22] == n and c[90:135].sum() == n
    assert [int(c[a:b].sum()) for a, b in BLOCKS] == [n] * 5
    # the farthest point (a corner) is at the normalising distance: f4's last bin
    assert c[135 + 44] >= 1 and c[135:135 + 44].sum() == n - c[135 + 44]
    # the centroid and the dominant normal: the patch's middle, the plane's normal towards the origin
    assert np.allclose(r.centroids[0], [0.3 + 0.004 * 9.5, 0.2 + 0.004 * 9.5, 1.0], atol=1e-6)
    assert np.allclose(r.dominant_normals[0], [0, 0, -1], atol=1e-6)
    # increments of 1: the row is its counts
    assert np.array_equal(r.rows[0], c.astype(np.float32))


def test_normalized_rows_are_sequential_sums(ref):
    s = flat_patch(11)
    n = len(s[0])
    r = R.cvfh(ref, O.normals, *s, prm=R.params(normalize_bins=True))
    shape, vp = F(100.0) / F(n - 1), F(100.0 / n)
    for b in range(308):
        want = R.sequential_sum(shape if b < 180 else vp, r.counts[0][b])
        assert r.rows[0][b].view(np.uint32) == want.view(np.uint32), b
    assert r.counts[0].max() > 16      # (a sum long enough to round)


def test_clusters_agree_with_union_find(ref, roof):
    prm = R.params()
    fx, fy, fz = R.filtered(ref, roof[0], roof[1], roof[2], roof[6], None, prm)
    assert 100 < len(roof[0]) - len(fx) < 600
    fn = O.normals(fx, fy, fz, float(prm.radius_normals))[:3]
    got = R.smooth_clusters(ref, fx, fy, fz, *fn, prm.cluster_tolerance, float(prm.eps_angle_threshold), 50)
    want = K.union_find_labels(fx, fy, fz, *fn, prm.cluster_tolerance, float(prm.eps_angle_threshold), 50)
    assert got.clusters == 2 and np.array_equal(got.labels, want)
    assert np.bincount(got.labels[got.labels >= 0]).min() >= 1400
    # the whole descriptor gives the same labels, scattered back to the indexed points
    r = R.cvfh(ref, O.normals, *roof)
    kept = ~(roof[6] > prm.curvature_threshold)
    assert np.array_equal(r.labels[kept], want) and set(r.labels[~kept]) == {-1}
    assert r.stats["cvfh_edges"] == got.edges and r.stats["cvfh_cc_rounds"] == got.rounds > 1


@pytest.mark.parametrize("eps", [0.125, 1e-3, 3.0])
def test_bisected_threshold_agrees_with_acos(ref, eps):
    T = F(ref.cvfh_acos_threshold(eps))
    assert -1.0 < T < 1.0
    v = T
    for _ in range(2000):
        assert ref.cvfh_smooth(float(v), eps) == 1 and np.arccos(np.float64(v)) < eps
        v = K.next_f32(v)
        if v > 1.0:
            break
    v = K.next_f32(T, False)
    for _ in range(2000):
        assert ref.cvfh_smooth(float(v), eps) == 0 and not np.arccos(np.float64(v)) < eps
        v = K.next_f32(v, False)
    # the ends: everything passes beyond pi, nothing at or below 0, and 1 < dot never
    assert ref.cvfh_acos_threshold(4.0) == -1.0 and ref.cvfh_acos_threshold(0.0) == np.inf
    assert ref.cvfh_smooth(float(K.next_f32(1.0)), 4.0) == 0 and ref.cvfh_smooth(float("nan"), 4.0) == 0


def test_min_points_and_fallback(ref):
    xyz, which = K.islands((49, 50, 51))
    s = xyz + K.flat_normals(150)
    r = R.cvfh(ref, O.normals, *s)
    assert r.stats["cvfh_clusters"] == 2 and [set(r.labels[which == k]) for k in range(3)] == [{-1}, {0}, {1}]
    r = R.cvfh(ref, O.normals, *s, prm=R.params(min_points=52))
    assert r.stats["cvfh_clusters"] == 0 and r.required == 1 and set(r.labels) == {-1}
    # the fallback's centroid is the surface's, its normal the mean of the normals, not normalised
    p = np.stack(xyz, 1).astype(np.float64)
    assert np.allclose(r.centroids[0], p.mean(0), atol=1e-5) and r.dominant_normals[0].tolist() == [0, 0, -1]
    # a capacity one short: the required count and nothing else
    r = R.cvfh(ref, O.normals, *s, cap=1)
    assert r.required == 2 and len(r.rows) == 0
