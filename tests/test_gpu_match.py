"""GPU parity: descriptor matching (Features<T>::getCorrespondences / findCorrespondences,
features.h:224-273) through the C-ABI against the CPU restatement (oracle/or_match.cpp).

Bar: bit-exact -- the same nearest row for every query in both directions, the same float
distance bits (FLANN L2_Simple order), the same correspondence list.  Covers FPFH-33 and
SHOT-352 sized rows, sizes off the 128-row tile, the PointCloud<SHOT352> stride (361 floats),
duplicated rows (ties), non-finite rows, empty inputs, and real FPFH descriptors of the
reference's clouds."""
import os

import numpy as np
import pytest

import oracle_lib as O
from match_data import pair, shot_like
from match_gpu import _check, _gpu_nearest, _same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,ns,nt", [("fpfh", 133, 151), ("fpfh", 1000, 777), ("shot", 300, 513),
                                        ("shot", 2049, 1500), ("shot", 2200, 2300)])
def test_match_parity(ctx, kind, ns, nt):
    """(2200 x 2300: over 16 tiles each way, so the seeding cross runs before the bound pass.)"""
    src, tgt = pair(kind, ns, nt, seed=ns + nt)
    assert _check(ctx, src, tgt) > 0
    if ns > 2048 and nt > 2048:
        assert 0 < ctx.stat("match_pairs_emitted") <= 64 * (ns + nt)


def test_match_shot352_stride(ctx):
    src, tgt = pair("shot", 260, 300, seed=9)
    _check(ctx, src, tgt, stride=361)


def test_match_ties_nonfinite_empty(ctx):
    rng = np.random.default_rng(11)
    tgt = shot_like(rng, 300)
    tgt[150:200] = tgt[0:50]       # duplicated rows: lowest row wins, both directions
    tgt[7, 11] = np.nan
    src = np.concatenate([tgt[100:260], shot_like(rng, 40)])
    src[5, 0] = np.inf
    _check(ctx, src, tgt)
    assert ctx.correspondences(src, tgt[:0])[0].size == 0
    assert ctx.correspondences(src[:0], tgt)[0].size == 0
    same = shot_like(rng, 64)      # identical sets: every row its own match
    q, m = ctx.correspondences(same, same)
    assert np.array_equal(q, np.arange(64)) and np.array_equal(m, q)


def test_match_real_fpfh_descriptors(ctx):
    """FPFH of the reference's indoor source/target clouds (restatement), keypoints = every
    53rd point: the matching the evaluation loop runs on (evaluation.cpp:342)."""
    from pcl_feature_extraction_amd.pcd import read_pcd
    desc = []
    for name in ("indoor_source", "indoor_target"):
        c = read_pcd(os.path.join(os.path.dirname(__file__), "golden", "clouds", name + ".pcd"))
        x, y, z = c.x[::3].copy(), c.y[::3].copy(), c.z[::3].copy()
        nx, ny, nz, _ = O.normals(x, y, z, 0.05)
        q = np.arange(0, len(x), 53)
        desc.append(O.fpfh(x, y, z, nx, ny, nz, x[q], y[q], z[q], 0.08))
    _check(ctx, desc[0], desc[1])


def test_nearest_host_api(ctx):
    """pfx_nearest_descriptors (host pointers, one direction: what the facade's
    KdTreeFLANN<FeatureT>::nearestKSearch calls)."""
    src, tgt = pair("fpfh", 700, 900, seed=5)
    src[3, 4] = np.nan
    idx, dist = ctx.nearest_descriptors(src, tgt)
    oi, od = O.nearest_descriptor(src, tgt)
    assert np.array_equal(idx, oi) and _same(dist, od)


def test_match_pair_list_overflow(ctx):
    """Near-duplicate sets (two distinct rows, 1000 copies each): every same-class pair ties, the
    bound pass's pruned pair list overflows, and the two-contraction fallback (candidates against
    the final bounds) must give the same answer."""
    rng = np.random.default_rng(21)
    base = shot_like(rng, 2)
    src = base[rng.integers(0, 2, 2000)]
    tgt = base[rng.integers(0, 2, 2000)]
    _gpu_nearest(ctx, src, tgt)
    # (the emission count is a 64-bit counter of every emitted pair: past the cap once the list
    # has overflowed)
    assert ctx.stat("match_pair_cap") == 64 * (len(src) + len(tgt)) + 65536
    assert ctx.stat("match_pairs_emitted") > ctx.stat("match_pair_cap")
    _check(ctx, src, tgt)
    # (the correspondences' second call goes straight to the two-contraction path: cap 0)
    assert ctx.stat("match_pairs_emitted") > ctx.stat("match_pair_cap")
