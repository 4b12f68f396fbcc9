"""The SPFH stage's point and pair counts on clusters of known size (63 / 64 / 65 / 129 / 200
mutually neighbouring points, and one cluster spread over several cells), rows equal to the CPU
restatement on raw float32 bits.  Support-only normals: with few queries on a large surface only
the cells around the queries are copied into the cell-ordered normal array; what an earlier call
left outside them is never read."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

R = 0.05


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _unit_normals(n, rng):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return [np.ascontiguousarray(v[:, i], dtype=np.float32) for i in range(3)]


def _ball(k, centre, radius, rng):
    d = rng.normal(size=(k, 3))
    d *= (radius * rng.uniform(0.02, 1.0, size=(k, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    return np.asarray(centre) + d


def _d2(q, p):
    """FLANN's float32 squared distance ((0 + dx^2) + dy^2) + dz^2 of every q to every p"""
    d = q[:, None, :].astype(np.float32) - p[None, :, :].astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(57)
    sizes = [63, 64, 65, 129, 200]
    # tiny clusters (radius 0.04 r: one grid cell, every point a neighbour of every other), 10 r
    # apart, and one cluster of 130 spread over 0.9 r: several cells, so several runs of its block
    pts = [_ball(k, (0.2 + 10 * R * i, -0.3, 1.0), 0.04 * R, rng) for i, k in enumerate(sizes)]
    pts.append(_ball(130, (0.2, -0.3 + 12 * R, 1.0), 0.9 * R, rng))
    first = np.cumsum([0] + [len(p) for p in pts[:-1]])
    p = np.concatenate(pts).astype(np.float32)
    xyz = [np.ascontiguousarray(p[:, i]) for i in range(3)]
    nrm = _unit_normals(len(p), rng)
    q = p[first]
    rr = np.float32(R * R)
    near = _d2(q, p) < rr
    s = np.flatnonzero(near.any(axis=0))                 # S: the r-neighbourhoods of the queries
    k = (_d2(p[s], p) < rr).sum(axis=1)                  # |N(p)|, the point itself included
    assert abs(_d2(p[s], p) / rr - 1).min() > 1e-5       # no distance near enough to r to be in doubt
    qs = [np.ascontiguousarray(q[:, i]) for i in range(3)]
    want = O.fpfh(*xyz, *nrm, *qs, R)
    assert not np.isnan(want).any()
    return xyz, nrm, qs, want, len(s), int((k - 1).sum())


@pytest.mark.parametrize("slow_cap", [None, "4"])
def test_spfh_counts(ctx, case, monkeypatch, slow_cap):
    xyz, nrm, qs, want, n_s, pairs = case
    if slow_cap:
        monkeypatch.setenv("PFX_FPFH_SLOW_CAP", slow_cap)
    got = ctx.fpfh(*xyz, *nrm, *qs, R)
    assert ctx.stat("fpfh_spfh_points") == n_s
    assert ctx.stat("fpfh_spfh_pairs") == pairs
    if slow_cap:
        assert ctx.stat("fpfh_spfh_exact_pairs") <= 4
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
    assert len(bad) == 0, f"rows {bad.tolist()} differ from the oracle"


def _slab(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform((0, 0, 1.0), (1.2, 1.2, 1.0 + 0.1), size=(n, 3)).astype(np.float32)
    return p, _unit_normals(n, rng)


def _pipeline_call(c, p, nrm, q):
    """fpfh_dev as the pipeline calls it: grid, S and keys prepared, the 2r support mask handed over"""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    s = [t(p[:, i]) for i in range(3)]
    n = [t(a) for a in nrm]
    qd = [t(q[:, i]) for i in range(3)]
    mask = torch.empty(len(p), dtype=torch.uint8, device=dev)
    out = torch.full((len(q), 33), 7.0, device=dev)
    c.fpfh_prepare_dev(*s, R)
    c.fpfh_prepare_queries_dev(*s, *qd, R)
    c.fpfh_support_ball_dev(*s, *qd, R, mask)
    c.fpfh_dev(*s, *n, *qd, R, out)
    c.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_support_only_normals():
    import torch
    from pcl_feature_extraction_amd import Context
    n = 200_000  # 40 queries: few enough for the copy of the queries' cells only (nq * 4096 <= n)
    (pa, na), (pb, nb) = _slab(n, 71), _slab(n, 72)
    qa, qb = pa[::5000].copy(), pb[2500::5000].copy()
    assert len(qb) * 4096 <= n
    want = O.fpfh(*[pb[:, i].copy() for i in range(3)], *nb, *[qb[:, i].copy() for i in range(3)], R)
    # every normal farther than 2r from all queries (with a margin over the float distance) -> NaN
    far = _d2(pb, qb).min(axis=1) > np.float32(4 * R * R * 1.001)
    assert 0.2 < far.mean() < 0.95
    nb_nan = [np.where(far, np.float32(np.nan), a) for a in nb]
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        _pipeline_call(c, pa, na, qa)            # leaves A's normals in the cell-ordered copy
        after_a = _pipeline_call(c, pb, nb, qb)
        with_nan = _pipeline_call(c, pb, nb_nan, qb)
        x, y, z = (pb[:, i].copy() for i in range(3))
        host_nan = c.fpfh(x, y, z, *nb_nan, *[qb[:, i].copy() for i in range(3)], R)
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        fresh = _pipeline_call(c, pb, nb, qb)
    assert not np.isnan(want).any()
    for name, got in (("fresh context", fresh), ("after cloud A", after_a), ("far normals NaN", with_nan),
                      ("far normals NaN, unprepared", host_nan)):
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
        assert len(bad) == 0, f"{name}: rows {bad[:8].tolist()} of {len(want)} differ"
