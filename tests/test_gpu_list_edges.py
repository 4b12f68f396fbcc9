"""GPU parity at the exact capacity edges of the neighbour-list build (pfx_nblist.hip), of the chain
consumer's four modes (pfx_normals.hip chain_wg) and of the consumers with caps of their own (SHOT,
FPFH weighting, radius search): every list sits at a capacity, one below it or one above it
(tests/list_edge_clouds.py; the constructions are proven on the CPU by test_list_edge_clouds.py).

All comparisons are raw float32 bits against the CPU restatement, as in test_gpu_features.py.
A fresh context's first estimation outgrows its first list buffer on most of these clouds and is
redone by the exact (32-bit-entry) path, so full-cloud estimations run twice on one context: the
second build stands as the deferred compact (16-bit-entry) build, and both must be exact.
"""
import numpy as np
import pytest

import list_edge_clouds as E
import oracle_lib as O
from pcl_feature_extraction_amd import Context, PfxError

pytestmark = pytest.mark.gpu

R = E.R
TILE_CAPS = (16, 384, 512, 1024, 2048, 4096)
PAIRS = [(100, 384), (100, 385), (100, 1280), (100, 1281), (100, 8000), (100, 8001), (600, 1280)]
TIERS = ["normals_tiles_sparse", "normals_tiles_dense", "normals_wide", "normals_single", "normals_mid8",
         "normals_mid", "normals_huge"]
CHAIN_MODES = ["staged", "deferred", "table", "lane"]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got, ref, what=""):
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = _bits(a), _bits(b)
        assert a.shape == b.shape
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, f"{what} output {i}: {len(bad)} rows differ, first {bad[:8]}"


def _stats(c, names):
    s = {nm: c.stat(nm) for nm in names}
    print({k.replace("normals_", ""): v for k, v in s.items()})
    return s


def _normals_twice(c, xyz, ref, what):
    """Exact path (or a standing first build), then a deferred compact build that stands."""
    g = c.normals(*xyz, R)
    _same_bits(g, ref, what + " (first build)")
    reruns = c.stat("normals_speculative_reruns")
    g = c.normals(*xyz, R)
    assert c.stat("normals_speculative_reruns") == reruns, "the second build was redone"
    _same_bits(g, ref, what + " (compact build)")


def _unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v.astype(np.float32)
    return v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0)) for a in arrays]


def _torch_stream(c):
    import torch
    c.set_stream(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)


@pytest.fixture(scope="module")
def tile_cloud():
    xyz, blobs = E.exact_k_blobs(TILE_CAPS)
    return xyz, blobs, O.normals(*xyz, R)


def _subset_normals(c, xyz, rows):
    """normals_subset_dev of `rows`: (outputs at rows, outputs elsewhere)."""
    import torch
    n = len(xyz[0])
    mask = np.zeros(n, np.uint8)
    mask[rows] = 1
    dx, dy, dz, dm = _dev(*xyz, mask)
    out = [torch.full((n,), 123.0, dtype=torch.float32, device=dx.device) for _ in range(4)]
    torch.cuda.synchronize()
    c.normals_subset_dev(dx, dy, dz, R, dm, 1, *out)
    c.synchronize()
    out = [o.cpu().numpy() for o in out]
    return [o[rows] for o in out], [np.delete(o, rows) for o in out]


def test_tile_and_per_query_edges(tile_cloud):
    """kQ = 16 queries per tile, kTcapSmall = 384 candidates, 512 / 1024 neighbours per tile query
    (1024 = kLongList), kLaneMaxCompact = kLaneMax = 2048, kCapQuery = 4096: blobs of cap - 1, cap,
    cap + 1 points, every point a query."""
    xyz, blobs, ref = tile_cloud
    n = len(xyz[0])
    with Context(0) as c:
        _normals_twice(c, xyz, ref, "tile edges")
        s = _stats(c, TIERS + ["normals_neighbors", "normals_queries", "normals_long_queries"])
    assert s["normals_neighbors"] == 1 + sum(k * k for k, _, _ in blobs)
    assert s["normals_queries"] == n
    assert s["normals_long_queries"] == sum(k for k, _, _ in blobs if k > 1024)
    assert s["normals_single"] > 0 and s["normals_mid8"] > 0   # (the 4097 blob: the 4k-8k tier)


def test_candidate_class_edges():
    """kTcapSmall / kTcapSparse / kTcapDense = 384 / 1280 / 8000 candidates per tile, each at the cap
    and one past it, with lists of 100 entries; (100, 1280) and (600, 1280) hold lists of 1180 and
    680 entries in a sparse-class tile (512 per query): the overflow hand-off to the per-query tier."""
    xyz, pairs = E.two_blob_blocks(PAIRS)
    ref = O.normals(*xyz, R)
    with Context(0) as c:
        _normals_twice(c, xyz, ref, "candidate classes")
        s = _stats(c, TIERS + ["normals_neighbors", "normals_queries"])
    assert s["normals_neighbors"] == 1 + sum(k_a * k_a + (t - k_a) ** 2 for k_a, t, _, _ in pairs)
    assert s["normals_queries"] == len(xyz[0])
    assert s["normals_tiles_sparse"] > 0 and s["normals_tiles_dense"] > 0 and s["normals_wide"] > 0
    assert s["normals_single"] > 0


def test_8k_16k_huge_edges_selected_rows():
    """kCapMid8 = 8192, kCapMid = 16384 and 65536 (the first counts that do not fit 16 bits), each
    -1 / 0 / +1: three queries per blob through normals_subset_dev."""
    xyz, blobs = E.exact_k_blobs((8192, 16384, 65536))
    rows = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    ref = O.normals_rows(*xyz, R, rows)
    with Context(0) as c:
        _torch_stream(c)
        got, rest = _subset_normals(c, xyz, rows)
        s = _stats(c, TIERS + ["normals_neighbors", "normals_queries", "normals_long_queries"])
    _same_bits(got, ref, "8k/16k/huge rows")
    for o in rest:
        assert (o == 123.0).all()   # the other outputs are left untouched
    assert s["normals_queries"] == len(rows) == s["normals_long_queries"]
    assert s["normals_neighbors"] == 3 * sum(k for k, _, _ in blobs)
    assert s["normals_mid8"] > 0 and s["normals_mid"] > 0 and s["normals_huge"] > 0


def test_capacity_edge_and_error():
    """kCapHuge = 262144: a list of exactly that many entries is exact, one more raises
    PFX_ERR_CAPACITY, and the context estimates exactly afterwards."""
    xyz, blobs = E.exact_k_blobs((262144,), deltas=(0,))
    rows = np.array(E.three_rows(*blobs[0][1:]))
    ref = O.normals_rows(*xyz, R, rows)
    over, oblobs = E.exact_k_blobs((262144,), deltas=(1,))
    orows = np.array(E.three_rows(*oblobs[0][1:]))
    small, _ = E.exact_k_blobs((16,))
    with Context(0) as c:
        _torch_stream(c)
        got, _ = _subset_normals(c, xyz, rows)
        _same_bits(got, ref, "262144 rows")
        assert c.stat("normals_huge") == 3 and c.stat("normals_neighbors") == 3 * 262144
        with pytest.raises(PfxError) as e:
            _subset_normals(c, over, orows)
        assert e.value.code == 3   # PFX_ERR_CAPACITY, as test_gpu_harris.py's capacity case
        _same_bits(c.normals(*small, R), O.normals(*small, R), "after the capacity error")


def test_tied_distances():
    """Lists whose d2 values are (nearly) all equal: one or two sort buckets hold the whole list
    and the caller-index tie-break orders it, at 513 / 1025 / 4097 / 16385 entries (tied shells) and
    17 / 385 / 513 / 1025 (identical points)."""
    shells, idents = (513, 1025, 4097, 16385), (17, 385, 513, 1025)
    xyz, groups = E.ties_cloud(shells, idents)
    x, y, z = xyz
    ref = O.normals(*xyz, R)
    with Context(0) as c:
        _normals_twice(c, xyz, ref, "ties")
        for k, lo, _ in groups:   # a shell's centre / one of the identical points
            cap = k + 8
            cg, ig, dg = c.radius_search(x, y, z, x[lo:lo + 1], y[lo:lo + 1], z[lo:lo + 1], R, cap=cap)
            cr, ir, dr = O.radius_search(x, y, z, x[lo:lo + 1], y[lo:lo + 1], z[lo:lo + 1], R, cap=cap)
            assert cg[0] == cr[0] == k
            assert np.array_equal(ig[0, :k], ir[0, :k]), k
            assert np.array_equal(_bits(dg[0, :k]), _bits(dr[0, :k])), k


def test_strict_radius_on_exact_floats():
    """A lattice whose coordinates and distances are exact in float32, neighbours at exactly r
    included: d2 < r * r is strict, 251 neighbours per interior point by counting integer vectors."""
    (x, y, z), inner = E.binary_lattice()
    r = E.LATTICE_R
    cap = 256
    with Context(0) as c:
        cg, ig, dg = c.radius_search(x, y, z, x, y, z, r, cap=cap)
        g = c.normals(x, y, z, r)
    assert (cg[inner] == E.LATTICE_INTERIOR_COUNT).all()
    cr, ir, dr = O.radius_search(x, y, z, x, y, z, r, cap=cap)
    assert np.array_equal(cg, cr) and cr.max() <= cap
    for j in range(len(x)):
        assert np.array_equal(ig[j, :cr[j]], ir[j, :cr[j]]), j
        assert np.array_equal(_bits(dg[j, :cr[j]]), _bits(dr[j, :cr[j]])), j
    _same_bits(g, O.normals(x, y, z, r), "lattice")


def test_chain_modes_all_reached(tile_cloud):
    """k_normals_chain's four modes under a parity check (the counters are published under
    per-kernel timing): per-lane run starts (> kMaxCells = 64 cells in a workgroup's 256 queries),
    the table with global bases (a union past kStageBig = 12288), deferral to k_normals_chain_big
    (a union past kStageSmall = 3584) and plain staging.  Measured (workgroups staged / deferred /
    table / lane): lattice 0 / 0 / 0 / 38, wide cube 48 / 51 / 3 / 0, tile-edge blobs 95 / 51 / 0 / 0."""
    names = ["normals_chain_wg_" + m for m in CHAIN_MODES]
    seen = {}

    def run(what, xyz, ref):
        with Context(0) as c:
            c.set_timing(True)
            _same_bits(c.normals(*xyz, R), ref, what)
            seen[what] = _stats(c, names)
        return seen[what]

    lattice = E.one_per_cell_lattice()
    s = run("lattice", lattice, O.normals(*lattice, R))
    assert s["normals_chain_wg_lane"] > 0
    wide, _ = E.assemble([np.random.default_rng(29).uniform(0, 0.15, (13000, 3)) + [10, 10, 1]])
    s = run("wide cube", wide, O.normals(*wide, R))
    assert s["normals_chain_wg_table"] > 0 or s["normals_chain_wg_deferred"] > 0
    xyz, _, ref = tile_cloud
    s = run("tile edges", xyz, ref)
    assert s["normals_chain_wg_deferred"] > 0 and s["normals_chain_wg_staged"] > 0
    for nm in names:
        assert any(v[nm] > 0 for v in seen.values()), nm


def test_mixed_entry_widths_reused_by_fpfh():
    """A compact build in which 16-bit lists (the 2047 / 2048 blobs) sit beside 32-bit ones: lists
    over kLaneMaxCompact = 2048 entries (2049, 5000) and short lists whose block has a run of more
    than 4096 points (the 100-point blob beside the 5000-point one); the normals' chains and FPFH's
    all-points weighting (which reuses the lists) read both widths."""
    import torch
    rng = np.random.default_rng(106)
    sparse, dense = E.dense_run_beside_sparse()
    xyz, rows = E.assemble([sparse, dense] + [E.exact_k_blob(rng, k, s) for s, k in enumerate((2047, 2048, 2049))])
    n = len(xyz[0])
    ref = O.normals(*xyz, R)
    dx, dy, dz = _dev(*xyz)
    nrm = [torch.empty(n, dtype=torch.float32, device=dx.device) for _ in range(4)]
    out = torch.empty((n, 33), dtype=torch.float32, device=dx.device)
    with Context(0) as c:
        _torch_stream(c)
        c.normals_dev(dx, dy, dz, R, *nrm)       # (outgrows the fresh list buffer: the exact path)
        torch.cuda.synchronize()
        _same_bits([a.cpu().numpy() for a in nrm], ref, "mixed widths (first build)")
        reruns = c.stat("normals_speculative_reruns")
        c.normals_dev(dx, dy, dz, R, *nrm)       # the compact build stands
        assert c.stat("normals_speculative_reruns") == reruns
        c.fpfh_dev(dx, dy, dz, *nrm[:3], dx, dy, dz, R, out, same_as_surface=True, after_normals=True)
        torch.cuda.synchronize()
        assert c.stat("fpfh_weight_lists_reused") == 1
        _same_bits([a.cpu().numpy() for a in nrm], ref, "mixed widths (compact build)")
        got = out.cpu().numpy()
    want = O.fpfh(*xyz, ref[0], ref[1], ref[2], *xyz, R, same_as_surface=True)
    for lo, hi in rows:
        _same_bits([got[lo:hi]], [want[lo:hi]], f"fpfh rows {lo}:{hi}")
    _same_bits([got], [want], "fpfh")


def test_shot_own_caps():
    """SHOT's kChunk = 256, kCapSmall = 2048 and kCap = 16384 neighbours: exact from 255 to 16384;
    one more is beyond SHOT's capacity and raises PFX_ERR_CAPACITY."""
    xyz, blobs = E.exact_k_blobs((256, 2048, 16384))
    nrm = _unit_normals(len(xyz[0]), 107)
    x, y, z = xyz
    q = np.array([r for k, lo, hi in blobs if k <= 16384 for r in E.three_rows(lo, hi)])
    qo = np.array([r for k, lo, hi in blobs if k > 16384 for r in E.three_rows(lo, hi)])
    assert len(q) == 24 and len(qo) == 3
    with Context(0) as c:
        desc, rf = c.shot(x, y, z, *nrm, x[q], y[q], z[q], R)
        with pytest.raises(PfxError) as e:
            c.shot(x, y, z, *nrm, x[qo], y[qo], z[qo], R)
        assert e.value.code == 3
        desc2, rf2 = c.shot(x, y, z, *nrm, x[q], y[q], z[q], R)   # and the context still works
    dref, rref = O.shot(x, y, z, *nrm, x[q], y[q], z[q], R)
    _same_bits([desc, rf], [dref, rref], "shot")
    _same_bits([desc2, rf2], [dref, rref], "shot after the capacity error")


def test_fpfh_weighting_own_cap():
    """FPFH's kCapW = 8192 neighbours of a query: the last list weighted in LDS and the first one
    weighted by the global-scratch pass."""
    xyz, blobs = E.exact_k_blobs((8192,), deltas=(0, 1))
    nrm = _unit_normals(len(xyz[0]), 108)
    x, y, z = xyz
    q = np.array([r for _, lo, hi in blobs for r in (lo, hi - 1)])
    with Context(0) as c:
        g = c.fpfh(x, y, z, *nrm, x[q], y[q], z[q], R)
        assert c.stat("fpfh_weight_global") >= 1
        assert c.stat("fpfh_weight_kmax") == 8193
    _same_bits([g], [O.fpfh(x, y, z, *nrm, x[q], y[q], z[q], R)], "fpfh weighting")


def test_radius_search_own_cap():
    """kCapSearch = 16384: lists of 16383 / 16384 ordered in LDS, 16385 by the overflow pass."""
    xyz, blobs = E.exact_k_blobs((16384,))
    x, y, z = xyz
    q = np.array([r for _, lo, hi in blobs for r in E.three_rows(lo, hi)])
    cap = 16392
    with Context(0) as c:
        cg, ig, dg = c.radius_search(x, y, z, x[q], y[q], z[q], R, cap=cap)
    cr, ir, dr = O.radius_search(x, y, z, x[q], y[q], z[q], R, cap=cap)
    assert list(cr) == [k for k, _, _ in blobs for _ in range(3)]
    assert np.array_equal(cg, cr)
    for j in range(len(q)):
        assert np.array_equal(ig[j, :cr[j]], ir[j, :cr[j]]), j
        assert np.array_equal(_bits(dg[j, :cr[j]]), _bits(dr[j, :cr[j]])), j
