"""The constructions of list_edge_clouds.py reach the edges they claim -- CPU only (oracle + numpy).

tests/test_gpu_list_edges.py runs the product on these clouds; here the inputs themselves are
proven: blob sizes are exact neighbour counts, the two-blob pairs share a 3x3x3 block without
neighbouring each other, the sparse lattice spreads every 256 queries over more than 64 cells, and
the binary lattice pins the strict `<` of the radius test without trusting the oracle.
"""
import numpy as np
import pytest

import list_edge_clouds as E
import oracle_lib as O

# every group of capacities the GPU tests use
BLOB_CAPS = [
    ((16, 384, 512, 1024, 2048, 4096), (-1, 0, 1)),   # kQ, kTcapSmall, per-query 512 / 1024 (= kLongList), kLaneMax, kCapQuery
    ((8192, 16384, 65536), (-1, 0, 1)),               # kCapMid8 (= FPFH's kCapW), kCapMid (= kCapSearch), 16-bit counts
    ((256, 2048, 16384), (-1, 0, 1)),                 # SHOT's kChunk, kCapSmall, kCap
    ((262144,), (0, 1)),                              # kCapHuge and one past it
]
PAIRS = [(100, 384), (100, 385), (100, 1280), (100, 1281), (100, 8000), (100, 8001), (600, 1280)]


def _counts(xyz, rows, r=E.R):
    x, y, z = xyz
    rows = np.asarray(rows)
    return O.radius_search(x, y, z, x[rows], y[rows], z[rows], r)[0]


@pytest.mark.parametrize("caps,deltas", BLOB_CAPS, ids=lambda v: "-".join(map(str, v)))
def test_exact_k_blobs_have_exactly_k_neighbours(caps, deltas):
    xyz, blobs = E.exact_k_blobs(caps, deltas)
    assert [k for k, _, _ in blobs] == [c + d for c in caps for d in deltas]
    assert xyz[0][0] == 0 and xyz[1][0] == 0 and xyz[2][0] == 0
    p = np.stack(xyz, axis=1)
    for k, lo, hi in blobs:
        assert hi - lo == k
        assert list(_counts(xyz, E.three_rows(lo, hi))) == [k, k, k], k
        assert len(np.unique(E.cells(p[lo:hi]), axis=0)) == 1   # one cell: tiles of 16 consecutive rows of it
    assert _counts(xyz, [0])[0] == 1


def test_two_blob_blocks_share_a_block_but_no_neighbour():
    xyz, pairs = E.two_blob_blocks(PAIRS)
    p = np.stack(xyz, axis=1)
    for k_a, t, (a0, a1), (b0, b1) in pairs:
        assert (a1 - a0, b1 - b0) == (k_a, t - k_a)
        assert list(_counts(xyz, E.three_rows(a0, a1))) == [k_a] * 3
        assert list(_counts(xyz, E.three_rows(b0, b1))) == [t - k_a] * 3
        ca, cb = np.unique(E.cells(p[a0:a1]), axis=0), np.unique(E.cells(p[b0:b1]), axis=0)
        assert len(ca) == 1 and len(cb) == 1
        assert list(cb[0] - ca[0]) == [1, 1, 0]
        # nothing else in either block: T candidates exactly
        near = (np.abs(E.cells(p) - ca[0]) <= 2).all(axis=1)
        assert near.sum() == t


def test_dense_run_beside_sparse_shares_a_z_run():
    a, b = E.dense_run_beside_sparse()
    xyz, ((a0, a1), (b0, b1)) = E.assemble([a, b])
    p = np.stack(xyz, axis=1)
    ca, cb = np.unique(E.cells(p[a0:a1]), axis=0), np.unique(E.cells(p[b0:b1]), axis=0)
    assert len(ca) == 1 and len(cb) == 1 and list(cb[0] - ca[0]) == [0, 1, 1]
    assert b1 - b0 > 4096
    assert list(_counts(xyz, E.three_rows(a0, a1))) == [a1 - a0] * 3
    assert list(_counts(xyz, E.three_rows(b0, b1))) == [b1 - b0] * 3


def test_ties_cloud_lists_are_tied():
    shells, idents = (513, 1025, 4097, 16385), (17, 385, 513, 1025)
    xyz, groups = E.ties_cloud(shells, idents)
    x, y, z = xyz
    for k, lo, hi in groups:
        assert list(_counts(xyz, E.three_rows(lo, hi))) == [k] * 3
    k, lo, hi = groups[3]
    _, idx, d2 = O.radius_search(x, y, z, x[lo:lo + 1], y[lo:lo + 1], z[lo:lo + 1], E.R, cap=k)
    assert len(np.unique(d2[0])) < 1000          # a few hundred distinct d2 among 16385 entries
    assert idx[0, 0] == lo
    k, lo, hi = groups[-1]
    _, idx, d2 = O.radius_search(x, y, z, x[lo:lo + 1], y[lo:lo + 1], z[lo:lo + 1], E.R, cap=k)
    assert (d2[0] == 0).all() and np.array_equal(idx[0], np.arange(lo, hi))


def test_one_per_cell_lattice_spreads_queries_over_cells():
    x, y, z = E.one_per_cell_lattice()
    assert E.min_cells_per_group(x, y, z) > 64   # k_normals_chain's kMaxCells


def test_binary_lattice_pins_the_strict_radius():
    assert E.lattice_ball_count(4) == E.LATTICE_INTERIOR_COUNT == 251
    (x, y, z), inner = E.binary_lattice()
    assert len(inner) == 125
    for a in (x, y, z):   # exact in float32
        assert np.array_equal(a.astype(np.float64) * 64, np.round(a.astype(np.float64) * 64))
    c = O.radius_search(x, y, z, x[inner], y[inner], z[inner], E.LATTICE_R)[0]
    assert (c == 251).all()


def test_normals_rows_equals_normals():
    import os
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_small.npz"), allow_pickle=False)
    x, y, z = f["x"], f["y"], f["z"]
    rows = np.random.default_rng(9).choice(len(x), 200, replace=False)
    full = O.normals(x, y, z, 0.05)
    some = O.normals_rows(x, y, z, 0.05, rows)
    for a, b in zip(full, some):
        assert np.array_equal(a[rows].view(np.uint32), b.view(np.uint32))
    vp = (0.3, -1.0, 2.0)
    for a, b in zip(O.normals(x, y, z, 0.05, vp=vp), O.normals_rows(x, y, z, 0.05, rows, vp=vp)):
        assert np.array_equal(a[rows].view(np.uint32), b.view(np.uint32))
