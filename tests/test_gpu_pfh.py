"""PFH-125 (pfx_pfh / pfx_pfh_dev, pfx_pfh.hip) against the CPU restatement of PCL 1.7
PFHEstimation (tests/cpp/pfh_ref.cpp, pinned by tests/test_pfh_ref.py): raw bits of every row, NaN
rows included.  Shapes are the smallest that reach every path of the kernel: the LDS / global-
scratch switch at its exact capacity, wave-edge neighbourhood sizes, ties of the pair orientation
rule, the one-bin worst case of the counters, degenerate pairs."""
import os

import numpy as np
import pytest

import list_edge_clouds as E
import pfh_cases as C
import pfh_ref as P
from parity import bits, bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = os.path.join(ROOT, "tests", "golden", "clouds")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("pfh_ref"))


def rows_of(a, rows):
    return tuple(v[rows] for v in a)


def check(ctx, ref, xyz, nrm, q, r=C.R):
    """ctx.pfh == the restatement, bit for bit; returns the rows."""
    got = ctx.pfh(*xyz, *nrm, *q, r)
    want, pairs = P.pfh(ref, *xyz, *nrm, *q, r)
    assert got.shape == want.shape == (len(q[0]), 125)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(bad) == 0, f"rows {bad[:8].tolist()} of {len(want)} differ"
    assert ctx.stat("pfh_pairs") == pairs
    return got


@pytest.fixture(scope="module")
def indoor(ctx, ref):
    """Case 1, shared: indoor source, normals at 0.05, 64 seeded cloud rows + 3 other points."""
    from pcl_feature_extraction_amd.pcd import read_pcd
    c = read_pcd(os.path.join(CLOUDS, "indoor_source.pcd"))
    xyz = (c.x, c.y, c.z)
    nrm = ctx.normals(*xyz, 0.05)[:3]
    fin = np.flatnonzero(np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.z))
    rows = np.sort(np.random.default_rng(11).choice(fin, 64, replace=False))
    a, b = rows[0], rows[1]
    extra = np.array([[9.0e3, 9.0e3, 9.0e3],                                            # far outside: k = 0
                      [c.x[a] + 0.003, c.y[a] - 0.002, c.z[a] + 0.001],                 # beside a cloud point
                      [c.x[b] - 0.01, c.y[b] + 0.01, c.z[b]]], np.float32)
    q = tuple(np.concatenate([v[rows], extra[:, i]]).astype(np.float32) for i, v in enumerate(xyz))
    want, pairs = P.pfh(ref, *xyz, *nrm, *q, 0.08)
    return dict(xyz=xyz, nrm=nrm, q=q, want=want, pairs=pairs)


def test_reference_cloud(ctx, indoor):
    got = ctx.pfh(*indoor["xyz"], *indoor["nrm"], *indoor["q"], 0.08)
    assert bits_equal(got, indoor["want"])
    assert np.isnan(got[64]).all() and not np.isnan(got[:64]).any()
    assert ctx.stat("pfh_pairs") == indoor["pairs"] and indoor["pairs"] > 64 * 1000


def test_capacity_edges(ctx, ref):
    cap = ctx.stat("pfh_cap_lds")
    xyz, blobs = E.exact_k_blobs(caps=[cap], deltas=(-1, 0, 1))
    nrm = C.unit_normals(len(xyz[0]), 21)
    rows = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    check(ctx, ref, xyz, nrm, rows_of(xyz, rows), E.R)
    assert [k for k, _, _ in blobs] == [cap - 1, cap, cap + 1]
    # only the blob above the capacity takes the global-scratch pass
    assert ctx.stat("pfh_global") == 3 and ctx.stat("pfh_kmax") == cap + 1


def test_small_neighbourhoods_at_wave_edges(ctx, ref):
    ks = (1, 2, 3, 63, 64, 65)
    xyz, nrm, rows = C.concat([C.blob(k, (1.0 + s, 2.0, 3.0), 30 + 2 * s) for s, k in enumerate(ks)])
    got = check(ctx, ref, xyz, nrm, xyz)
    assert not got[rows[0][0]].any()                                   # k = 1: zeros, not NaN
    assert all(np.count_nonzero(got[r]) == 1 and got[r].max() == 100.0 for r in range(*rows[1]))  # k = 2
    assert ctx.stat("pfh_kmax") == 65


def test_orientation_ties_on_a_lattice(ctx, ref):
    xyz, nrm = C.lattice_patch()
    got = check(ctx, ref, xyz, nrm, xyz)
    # the orientation rule is exercised: f3 = +-angle1 lands on both sides of the middle f3 bin
    b3 = np.arange(125) // 25
    assert got[:, b3 < 2].any() and got[:, b3 > 2].any()


def test_plane_one_bin(ctx, ref):
    xyz, nrm = C.plane_patch()
    got = check(ctx, ref, xyz, nrm, xyz)
    assert (np.count_nonzero(got, axis=1) == 1).all() and (got[:, 62] != 0).all()


def test_degenerates(ctx, ref):
    (x, y, z), (nx, ny, nz) = C.blob(48, (1.0, 2.0, 3.0), 40)
    dup = np.arange(0, 48, 6)  # exact duplicates of 8 points (f4 == 0 pairs), normals of their own
    x, y, z = (np.concatenate([v, v[dup]]) for v in (x, y, z))
    extra = C.unit_normals(len(dup), 41)
    nx, ny, nz = (np.concatenate([v, e]) for v, e in zip((nx, ny, nz), extra))
    for i in (3, 17, 50):  # NaN normals, one of them on a duplicate
        nx[i] = ny[i] = nz[i] = np.nan
    ny[20] = np.nan        # partly NaN
    qx, qy, qz = (np.concatenate([v, np.float32([np.nan])]) for v in (x, y, z))
    qy[-1] = 2.0
    got = check(ctx, ref, (x, y, z), (nx, ny, nz), (qx, qy, qz))
    assert np.isnan(got[-1]).all() and not np.isnan(got[:-1]).any()
    # every point sees all k = 56: the 8 coincident pairs are missing from each row's sum (the
    # float additions of a row: at most 2^-18 each)
    c = 56 * 55 // 2
    assert np.abs(got[:-1].astype(np.float64).sum(axis=1) - 100.0 * (1 - 8 / c)).max() < c * 2.0 ** -18 + 1e-4

    empty = ctx.pfh(x, y, z, nx, ny, nz, x[:0], y[:0], z[:0], C.R)
    assert empty.shape == (0, 125)
    from pcl_feature_extraction_amd import PfxError
    with pytest.raises(PfxError):
        ctx.pfh(x, y, z, nx, ny, nz, x, y, z, 0.0)


def test_neighbourhood_beyond_every_capacity_is_reported(ctx):
    """k = 65536: the pair count no longer fits 32 bits -> PFX_ERR_CAPACITY (and a NaN row), at once
    from the host API; the next call on the context is unaffected."""
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    xyz, nrm = C.blob(65536, (1.0, 2.0, 3.0), 50)
    with pytest.raises(PfxError) as e:
        ctx.pfh(*xyz, *nrm, *rows_of(xyz, [0]), C.R)
    assert e.value.code == PFX_ERR_CAPACITY
    small, sn = C.blob(8, (1.0, 2.0, 3.0), 51)
    assert not np.isnan(ctx.pfh(*small, *sn, *small, C.R)).any()


def test_pfh_dev_stream_ordered_and_deterministic(indoor):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
         for a in (*indoor["xyz"], *indoor["nrm"], *indoor["q"])]
    nq = len(indoor["q"][0])
    outs = [torch.full((nq, 125), -1.0, dtype=torch.float32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()  # (the context runs on its own stream)
    with Context(0) as c:
        c.pfh_dev(*t, 0.08, outs[0])
        c.pfh_dev(*t, 0.08, outs[1])
        c.synchronize()
        c.trim()
        c.pfh_dev(*t, 0.08, outs[2])
        c.synchronize()
        assert c.stat("pfh_pairs") == indoor["pairs"]
    for o in outs:
        assert bits_equal(o.cpu().numpy(), indoor["want"])


def test_matching_at_dim_125(ctx, indoor):
    import oracle_lib as O
    from pcl_feature_extraction_amd.pcd import read_pcd
    t = read_pcd(os.path.join(CLOUDS, "indoor_target.pcd"))
    txyz = (t.x, t.y, t.z)
    tn = ctx.normals(*txyz, 0.05)[:3]
    fin = np.flatnonzero(np.isfinite(t.x) & np.isfinite(t.y) & np.isfinite(t.z))
    rows = np.sort(np.random.default_rng(12).choice(fin, 64, replace=False))
    tgt = ctx.pfh(*txyz, *tn, *rows_of(txyz, rows), 0.08)
    src = indoor["want"][:64]
    assert not np.isnan(tgt).any()
    q, m = ctx.correspondences(src, tgt)
    oq, om = O.correspondences(src, tgt)
    assert np.array_equal(q, oq) and np.array_equal(m, om) and len(q) > 0
