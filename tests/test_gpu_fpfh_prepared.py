"""FPFH keypoint weighting on keys sorted ahead (pfx_fpfh_prepare_queries_dev): the rows equal the
unprepared call's and the CPU restatement's on raw float32 bits, NaN rows included.

The cloud is one cluster per neighbour count k: k points within 0.3 r of a centre, centres 10 r
apart, so a query near a centre has exactly that cluster as its neighbourhood.  The counts sit
on the edges of the staging chunks: 128 rows without prepared keys, 128 * D with them (D = 2, the
depth of the prepared path's row buffers), and on both sides of one and of several chunks."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

R = 0.05
DEPTH = 2  # kStageDepth of pfx_fpfh.hip
COUNTS = sorted({1, 2, 127, 128, 129, 256, 257, 1025, 128 * DEPTH - 1, 128 * DEPTH, 128 * DEPTH + 1})


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _unit_normals(n, rng):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return [np.ascontiguousarray(v[:, i], dtype=np.float32) for i in range(3)]


def _clusters(counts, rng):
    """-> xyz (float32 columns), the first row of every cluster, the centres"""
    pts, first, centres = [], [], []
    n = 0
    for i, k in enumerate(counts):
        c = np.array([0.3 + 10 * R * (i % 4), -0.2 + 10 * R * (i // 4), 1.1])
        d = rng.normal(size=(k, 3))
        d *= (0.3 * R * rng.uniform(0.05, 1.0, size=(k, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(c + d)
        first.append(n)
        centres.append(c)
        n += k
    p = np.concatenate(pts).astype(np.float32)
    return [np.ascontiguousarray(p[:, i]) for i in range(3)], np.array(first), np.array(centres)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(41)
    xyz, first, centres = _clusters(COUNTS, rng)
    nrm = _unit_normals(len(xyz[0]), rng)
    # per cluster: its first point (a d2 == 0 neighbour, which PCL skips) and the displaced centre;
    # then a query far from everything (NaN row) and a non-finite one
    q = np.concatenate([np.stack([xyz[i][first] for i in range(3)], 1),
                        centres + np.array([0.11, -0.07, 0.05]) * R,
                        [[5.0, 5.0, 5.0]], [[np.nan, 0.0, 1.0]]]).astype(np.float32)
    qs = [np.ascontiguousarray(q[:, i]) for i in range(3)]
    want = O.fpfh(*xyz, *nrm, *qs, R)
    assert np.isnan(want[-2:]).all() and not np.isnan(want[:-2]).any()
    return xyz, nrm, qs, want


def _dev(arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)) for a in arrs]


def _run(c, s, n, q, prepare_for=None):
    """fpfh_dev, after a preparation for the queries `prepare_for` if given -> rows, prepared?"""
    import torch
    out = torch.full((q[0].numel(), 33), 7.0, device=q[0].device)
    if prepare_for is not None:
        c.fpfh_prepare_queries_dev(*s, *prepare_for, R)
    c.fpfh_dev(*s, *n, *q, R, out)
    c.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy(), c.stat("fpfh_weight_prepared")


def test_prepared_keys_equal_in_kernel_keys(case):
    import torch
    from pcl_feature_extraction_amd import Context
    xyz, nrm, qs, want = case
    s, n, q = _dev(xyz), _dev(nrm), _dev(qs)
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        plain, used = _run(c, s, n, q)
        assert used == 0
        prep, used = _run(c, s, n, q, prepare_for=q)
        assert used == 1
        assert c.stat("fpfh_weight_kmax") == max(COUNTS) and c.stat("fpfh_weight_global") == 0
        again, used = _run(c, s, n, q)  # one-shot: the preparation is spent
        assert used == 0
    for name, got in (("unprepared", plain), ("prepared", prep), ("after the preparation", again)):
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
        assert len(bad) == 0, f"{name}: rows {bad[:8].tolist()} of {len(want)} differ from the oracle"


def test_preparation_for_other_queries_is_not_used(case):
    import torch
    from pcl_feature_extraction_amd import Context
    xyz, nrm, qs, want = case
    s, n, q = _dev(xyz), _dev(nrm), _dev(qs)
    # the same values at another address, reversed: keys prepared for these must not be taken
    other = [t.flip(0).contiguous() for t in q]
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        got_ptr, used_ptr = _run(c, s, n, q, prepare_for=other)
        # the same pointer, another count
        got_cnt, used_cnt = _run(c, s, n, q, prepare_for=[t[:-3] for t in q])
        short = [t[:-3] for t in q]
        got_short, used_short = _run(c, s, n, short, prepare_for=q)
    assert used_ptr == 0 and used_cnt == 0 and used_short == 0
    assert np.array_equal(_bits(got_ptr), _bits(want))
    assert np.array_equal(_bits(got_cnt), _bits(want))
    assert np.array_equal(_bits(got_short), _bits(want[:-3]))


def test_prepared_overflow_query_takes_the_global_pass():
    """8,193 points in one ball (one more than the LDS key capacity) beside ~2k others: the
    prepared count sends the query to the global-scratch pass, rows as without preparation."""
    import torch
    from pcl_feature_extraction_amd import Context
    rng = np.random.default_rng(43)
    xyz, first, centres = _clusters([8193, 700, 900, 400], rng)
    nrm = _unit_normals(len(xyz[0]), rng)
    q = np.concatenate([centres + np.array([0.05, 0.02, -0.04]) * R,
                        np.stack([xyz[i][first] for i in range(3)], 1)]).astype(np.float32)
    s, n = _dev(xyz), _dev(nrm)
    qd = _dev([q[:, i] for i in range(3)])
    with Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        plain, used = _run(c, s, n, qd)
        assert used == 0 and c.stat("fpfh_weight_global") >= 1
        prep, used = _run(c, s, n, qd, prepare_for=qd)
        assert used == 1 and c.stat("fpfh_weight_global") >= 1 and c.stat("fpfh_weight_kmax") == 8193
    assert not np.isnan(prep).any()
    assert np.array_equal(_bits(prep), _bits(plain))
