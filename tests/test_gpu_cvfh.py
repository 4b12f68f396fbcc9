"""CVFH and the smooth clusters (pfx_cvfh, pfx_smooth_clusters and their _dev forms, pfx_cvfh.hip)
against the CPU restatement (tests/cpp/cvfh_ref.cpp, pinned by tests/test_cvfh_ref.py): rows,
centroids, dominant normals, labels and the five statistics, bit for bit.  There is no tolerance: every
output is a count or an ordered float sum.  Each test first asserts, on the restatement alone, the
condition that makes it a test."""
import os

import numpy as np
import pytest

import cvfh_cases as K
import cvfh_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

F = np.float32
STATS = ("cvfh_filtered", "cvfh_clusters", "cvfh_edges", "cvfh_cc_rounds", "cvfh_rows")
BLOCKS = ((0, 45), (45, 90), (90, 135), (135, 180), (180, 308))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clouds")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("cvfh_ref"))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def api_params(prm):
    from pcl_feature_extraction_amd import cvfh_params
    return cvfh_params(tuple(prm.viewpoint), prm.radius_normals, prm.cluster_tolerance, prm.eps_angle_threshold,
                       prm.curvature_threshold, prm.min_points, prm.normalize_bins)


def same(got, want, ctx=None):
    """A Context.cvfh result equals the restatement's, every bit; with ctx the statistics too."""
    assert got.rows.shape == want.rows.shape and got.labels.shape == want.labels.shape
    for name in ("rows", "centroids", "dominant_normals"):
        g, w = bits(getattr(got, name)), bits(getattr(want, name))
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{name}: {len(bad)} differ, first at {bad[0].tolist()}"
    assert np.array_equal(got.labels, want.labels)
    if ctx is not None:
        assert {s: ctx.stat(s) for s in STATS} == want.stats


def check(ctx, ref, surface, indices=None, prm=None):
    """Context.cvfh == the restatement; returns the restatement's result."""
    prm = prm or R.params()
    want = R.cvfh(ref, O.normals, *surface, indices=indices, prm=prm)
    got = ctx.cvfh(*surface, indices=indices, params=api_params(prm))
    same(got, want, ctx)
    return want


def with_normals(ctx, xyz, r=0.02):
    """xyz + Context.normals at r: the seven surface columns."""
    return tuple(xyz) + tuple(ctx.normals(*xyz, r))


def block_sums(counts):
    return [int(counts[a:b].sum()) for a, b in BLOCKS]


# ---- 1. the roof ----

@pytest.fixture(scope="module")
def roof(ctx, ref):
    s = with_normals(ctx, K.roof())
    return dict(surface=s, want=R.cvfh(ref, O.normals, *s))


def test_roof(ctx, roof):
    want = roof["want"]
    sizes = np.bincount(want.labels[want.labels >= 0])
    print("roof: clusters", sizes.tolist(), want.stats)
    # (on the restatement alone) two faces, the crease filtered
    assert want.stats["cvfh_clusters"] == 2 and sizes.min() >= 1400
    assert len(want.labels) - want.stats["cvfh_filtered"] > 100
    same(ctx.cvfh(*roof["surface"]), want, ctx)


def test_roof_partial_workgroups(ctx, ref):
    s = with_normals(ctx, K.roof(24))
    assert len(s[0]) % 256 != 0 and len(s[0]) > 256
    want = check(ctx, ref, s)
    assert want.stats["cvfh_clusters"] == 2 and np.bincount(want.labels[want.labels >= 0]).min() >= 450


# ---- 2. the strip: a label that travels ----

@pytest.mark.parametrize("order", ["index", "reverse", "shuffled"])
def test_strip(ctx, ref, order):
    xyz = K.strip(order=order)
    nrm = K.flat_normals(len(xyz[0]))[:3]
    want = R.smooth_clusters(ref, *xyz, *nrm, K.TOL, 0.125, 50)
    assert want.clusters == 1 and (want.labels == 0).sum() == 4500 and want.rounds > 1
    labels, n = ctx.smooth_clusters(*xyz, *nrm, K.TOL, 0.125, 50)
    assert n == 1 and np.array_equal(labels, want.labels)
    assert (ctx.stat("cvfh_edges"), ctx.stat("cvfh_cc_rounds"), ctx.stat("cvfh_clusters")) == \
        (want.edges, want.rounds, want.clusters)
    print("strip", order, "rounds", want.rounds)


def test_strip_descriptor(ctx, ref):
    xyz = K.strip(order="shuffled")
    want = check(ctx, ref, xyz + K.flat_normals(len(xyz[0])))
    assert want.stats["cvfh_clusters"] == 1 and want.stats["cvfh_cc_rounds"] > 1 and want.stats["cvfh_filtered"] == 4500


# ---- 3. the min_points edge ----

def test_min_points_edge(ctx, ref):
    xyz, which = K.islands((49, 50, 51))
    s = xyz + K.flat_normals(len(which))
    want = check(ctx, ref, s)
    assert want.stats["cvfh_clusters"] == 2 and len(want.rows) == 2
    assert set(want.labels[which == 0]) == {-1} and set(want.labels[which == 1]) == {0}
    assert set(want.labels[which == 2]) == {1}
    # no island reaches 52: the fallback row
    want = check(ctx, ref, s, prm=R.params(min_points=52))
    assert want.stats["cvfh_clusters"] == 0 and want.stats["cvfh_rows"] == 1 and set(want.labels) == {-1}
    assert block_sums(want.counts[0])[4] == 150


def test_filtered_cloud_below_min_points(ctx, ref):
    """|F| = 49 of P = 200: the fallback."""
    xyz, which = K.islands((49, 151), gap=0.1)
    nx, ny, nz, curv = K.flat_normals(200)
    curv = np.where(which == 1, F(0.5), F(0.0)).astype(np.float32)
    want = check(ctx, ref, xyz + (nx, ny, nz, curv))
    assert want.stats["cvfh_filtered"] == 49 and want.stats["cvfh_clusters"] == 0 and len(want.rows) == 1


def test_nothing_passes_the_filter(ctx, ref):
    xyz, _ = K.islands((60,))
    nx, ny, nz, curv = K.flat_normals(60)
    want = check(ctx, ref, xyz + (nx, ny, nz, curv + F(1.0)))
    assert want.stats["cvfh_filtered"] == 0 and len(want.rows) == 1


# ---- 4. the angle edge, 5. the distance edge: smooth_clusters with injected values ----

def pairs(normals, dx=0.01):
    """Pair k: a point at (k, 0, 0) with the normal (1, 0, 0) and one dx beside it with normals[k]."""
    n = len(normals)
    p = np.zeros((2 * n, 3), np.float32)
    nr = np.zeros((2 * n, 3), np.float32)
    nr[:, 0] = 1.0
    for k in range(n):
        p[2 * k, 0] = k
        p[2 * k + 1, 0] = F(k) + F(dx)
        nr[2 * k + 1] = normals[k]
    return tuple(p.T.copy()), tuple(nr.T.copy())


@pytest.mark.parametrize("eps", [0.125, 1e-3, 3.0])
def test_angle_edge(ctx, ref, eps):
    T = F(ref.cvfh_acos_threshold(eps))
    dots = [T, K.next_f32(T, False), F(1.0), K.next_f32(1.0), F(np.nan)]
    # (on the restatement alone) the float dot of (1, 0, 0) and (v, 0, 0) is v, and acos decides
    assert [ref.cvfh_smooth(float(d), eps) for d in dots] == [1, 0, 1, 0, 0]
    xyz, nrm = pairs([(d, 0, 0) for d in dots])
    want = R.smooth_clusters(ref, *xyz, *nrm, K.TOL, eps, 2)
    assert want.labels.tolist() == [0, 0, -1, -1, 1, 1, -1, -1, -1, -1] and want.edges == 2
    labels, n = ctx.smooth_clusters(*xyz, *nrm, K.TOL, eps, 2)
    assert n == 2 and np.array_equal(labels, want.labels) and ctx.stat("cvfh_edges") == 2


def test_distance_edge(ctx, ref):
    d = F(0.0151)                     # the tolerance and the first pair's distance
    tt = F(d * d)                     # (float)(t t): the product of the same operands, rounded once
    assert tt == F(float(d) * float(d))
    # a pair one ulp of d^2 below: dx = the float below d, dy found so that the float sum is it
    below, dx = K.next_f32(tt, False), K.next_f32(d, False)
    ulp = float(tt) - float(below)
    dy = next((c for c in (F(np.sqrt(k * ulp / 64)) for k in range(1, 512))
               if (F(0) + dx * dx) + c * c == below), None)
    assert dy is not None and (F(0) + dx * dx) + dy * dy < tt
    # (both pairs start at x = y = 0, so the differences are d, dx and dy themselves; z parts them)
    x = np.array([0, d, 0, dx], np.float32)
    y = np.array([0, 0, 0, dy], np.float32)
    z = np.array([0, 0, 1, 1], np.float32)
    o = np.zeros(4, np.float32)
    nrm = (np.ones(4, np.float32), o, o)
    want = R.smooth_clusters(ref, x, y, z, *nrm, d, 0.125, 2)
    assert want.labels.tolist() == [-1, -1, 0, 0] and want.edges == 1
    labels, n = ctx.smooth_clusters(x, y, z, *nrm, d, 0.125, 2)
    assert n == 1 and np.array_equal(labels, want.labels) and ctx.stat("cvfh_edges") == 1


# ---- 6. the curvature edge ----

def test_curvature_edge(ctx, ref):
    xyz, _ = K.islands((120,))
    nx, ny, nz, curv = K.flat_normals(120)
    thr = F(0.03)
    curv[0:120:3] = thr                    # kept
    curv[1:120:3] = K.next_f32(thr)        # dropped
    curv[2:120:6] = np.nan                 # kept
    want = check(ctx, ref, xyz + (nx, ny, nz, curv), prm=R.params(min_points=10))
    assert want.stats["cvfh_filtered"] == 80 and set(want.labels[1:120:3]) == {-1}
    assert (want.labels[0:120:3] >= 0).all() and (want.labels[2:120:3] >= 0).all()


# ---- 7. counts beyond a wave and a workgroup ----

def test_twenty_thousand_points(ctx, ref):
    s = with_normals(ctx, K.roof(100, 0.0025, 0.00025))
    assert len(s[0]) == 20000
    want = check(ctx, ref, s)
    assert want.stats["cvfh_clusters"] >= 2
    for row in want.counts:      # (a bin several workgroups of 256 add to)
        b = block_sums(row)
        assert b[4] == 20000 and b[0] == b[1] == b[2] == b[3] <= 20000 and max(row) > 4 * 256
    print("20,000 points:", want.stats)


@pytest.mark.parametrize("normalize", [False, True])
def test_three_faces(ctx, ref, normalize):
    s = with_normals(ctx, K.corner())
    want = check(ctx, ref, s, prm=R.params(normalize_bins=normalize))
    assert want.stats["cvfh_clusters"] >= 3
    for row in want.counts:
        assert block_sums(row) == [len(s[0])] * 5


# ---- 8. degenerate inputs ----

def test_point_at_the_centroid(ctx, ref):
    x, y = np.array([0, 1, -1], np.float32), np.array([0, 0.5, -0.5], np.float32)
    z = np.full(3, 2, np.float32)
    nx, ny, nz, curv = K.flat_normals(3)
    want = check(ctx, ref, (x, y, z, nx, ny, nz, curv))
    assert want.centroids.tolist() == [[0, 0, 2]] and block_sums(want.counts[0]) == [2, 2, 2, 2, 3]
    assert want.counts[0][135 + 44] == 2     # both at the largest distance: f4's last bin


def test_non_finite_points_and_normals(ctx, ref):
    s = [v.copy() for v in with_normals(ctx, K.roof(24))]
    s[0][5], s[1][17], s[2][40] = np.nan, np.inf, -np.inf
    s[3][60], s[4][61], s[5][62], s[6][70] = np.nan, np.nan, np.inf, np.nan
    want = check(ctx, ref, tuple(s))
    assert want.stats["cvfh_clusters"] == 2


def test_indices(ctx, ref, roof):
    s = roof["surface"]
    idx = np.random.default_rng(5).permutation(len(s[0]))[:2500].astype(np.int32)
    assert not np.all(np.diff(idx) > 0)
    want = check(ctx, ref, s, indices=idx)
    assert want.stats["cvfh_clusters"] >= 1 and len(want.labels) == 2500
    got = ctx.cvfh(*s, indices=np.zeros(0, np.int32))
    assert got.rows.shape == (0, 308) and got.labels.shape == (0,) and ctx.stat("cvfh_rows") == 0


def test_capacity(ctx, roof):
    from pcl_feature_extraction_amd import PfxError
    with pytest.raises(PfxError) as e:
        ctx.cvfh(*roof["surface"], cap=1)
    assert e.value.code == 3 and e.value.required == 2
    same(ctx.cvfh(*roof["surface"]), roof["want"], ctx)   # the context is usable afterwards


# ---- 9. the reference's cloud ----

def test_reference_cloud(ctx, ref):
    from pcl_feature_extraction_amd.pcd import read_pcd
    c = read_pcd(os.path.join(GOLDEN, "indoor_source.pcd"))
    s = with_normals(ctx, (c.x, c.y, c.z), 0.05)
    want = check(ctx, ref, s, indices=np.arange(2000, dtype=np.int32))
    print("indoor source, first 2,000 points:", want.stats)


# ---- 10. the forms ----

def test_forms(ctx, roof):
    import torch
    s, want = roof["surface"], roof["want"]
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in s]
    n = len(s[0])
    out = torch.empty((4, 308), dtype=torch.float32, device="cuda")
    cen, dn = (torch.empty((4, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    n_rows = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        ctx.cvfh_dev(*dev, None, out, n_rows, centroids=cen, dominant_normals=dn, labels=labels)
        ctx.synchronize()
        m = int(n_rows.cpu()[0])
        runs.append(R.Result(out[:m].cpu().numpy(), None, cen[:m].cpu().numpy(), dn[:m].cpu().numpy(),
                             labels.cpu().numpy(), None, m))
        assert {k: ctx.stat(k) for k in STATS} == want.stats
    same(runs[0], want)
    same(runs[1], want)


def test_cluster_forms(ctx):
    import torch
    xyz = K.strip(300, order="shuffled")
    nrm = K.flat_normals(len(xyz[0]))[:3]
    host, n_host = ctx.smooth_clusters(*xyz, *nrm, K.TOL, 0.125, 50)
    assert n_host == 1
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in xyz + nrm]
    labels = torch.empty(len(xyz[0]), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        ctx.smooth_clusters_dev(*dev, K.TOL, 0.125, 50, labels, n)
        ctx.synchronize()
        assert int(n.cpu()[0]) == 1 and np.array_equal(labels.cpu().numpy(), host)
