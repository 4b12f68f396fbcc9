"""The list set-up from the sorted positions (pfx_nblist.hip k_tile_cells) where its walk can go
wrong, and the normal estimation's forked coordinate gather (pfx_grid.hip build_grid).

A workgroup of k_tile_cells takes a slice of P = 4096 consecutive sorted positions (kSlice in
pfx_nblist.hip = 256 threads x kSlicePerThread 16); a cell belongs to the slice that holds its first
point.  The clouds put cell starts on both sides of a slice boundary, leave a slice without any
start, make every position a start, and end the finite points exactly on a boundary.

Layout (list_edge_clouds): the anchor at the origin is sorted position 0 and lies in the grid's
corner cell (0, 0, 0); the blobs follow in the order given (one cell each, ascending x cell), so
blob b starts at position 1 + the sizes before it.  Non-finite points sort behind every cell.

Every cloud: Context.normals twice (the exact path, then a deferred build) under
PFX_LIST_SETUP=cells and =scan, bit-for-bit against the oracle, and the tile statistics of the two
modes equal.
"""
import functools

import numpy as np
import pytest

import list_edge_clouds as E
import oracle_lib as O
from pcl_feature_extraction_amd import Context

pytestmark = pytest.mark.gpu

P = 4096  # kSlice


def _blobs(sizes, seed=201):
    rng = np.random.default_rng(seed)
    return E.assemble([E.exact_k_blob(rng, k, s) for s, k in enumerate(sizes)])[0]


def _with_non_finite(xyz, seed=202):
    """NaN / inf rows scattered through the caller's order (a NaN in one coordinate is enough)."""
    rng = np.random.default_rng(seed)
    x, y, z = (a.copy() for a in xyz)
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    at = np.sort(rng.choice(len(x) + 1, 37, replace=False))
    rows = bad[rng.integers(0, len(bad), len(at))]
    return tuple(np.insert(a, at, rows[:, d]).astype(np.float32) for d, a in enumerate((x, y, z)))


def _corners():
    """Occupied cells at two opposite grid corners: (0, 0, 0) and the last cell, whose 3x3x3 blocks
    are clipped on three sides each (the far blob's maximum is the grid's upper bound), and one cell
    in between touching neither."""
    rng = np.random.default_rng(203)
    parts = [E.cube(rng, 40, E.cell_centre(0, 0, 0), 0.02), E.cube(rng, 33, E.cell_centre(2, 2, 2), 0.02),
             E.cube(rng, 47, E.cell_centre(4, 4, 4), 0.02)]
    return E.assemble(parts)[0]


def _all_nan(n):
    return tuple(np.full(n, np.nan, np.float32) for _ in range(3))


CLOUDS = {
    # positions 1..4094 one cell; the next cell starts at 4095, the last position of slice 0
    "start on the last position of a slice": lambda: _blobs([P - 2, 20]),
    # ... and at 4096, the first position of slice 1
    "start on the first position of a slice": lambda: _blobs([P - 1, 20]),
    # 1 + 1500 + 2595 = 4096 finite points: the last slice is full, no partial one follows
    "finite count a multiple of P": lambda: _blobs([1500, P - 1501]),
    # the 9000-point cell starts at 101 and ends at 9101: slice 1 (4096..8191) holds no start; its
    # 563 tiles (> 16) all belong to slice 0's workgroup
    "a slice without a start": lambda: _blobs([100, 9000, 50]),
    # three positions in four start a cell (9601 points, 7407 cells of at most 6) ...
    "most positions a start": E.one_per_cell_lattice,
    # ... and every one: 0.06 apart and jittered by 0.004, no two points share a 0.05 cell (nor lie
    # within R of each other: every list is the point itself), 4609 > P points
    "every position a start": lambda: E.one_per_cell_lattice(spacing=0.06, dims=(24, 24, 8)),
    "a very full cell beside sparse ones": lambda: E.assemble(list(E.dense_run_beside_sparse()))[0],
    # 37 non-finite rows: they sort behind every cell (positions >= 4115) and start no tile
    "non-finite points": lambda: _with_non_finite(_blobs([P - 2, 20])),
    "all points non-finite": lambda: _all_nan(300),
    "n = 1": lambda: tuple(np.array([v], np.float32) for v in (0.5, 0.25, 0.125)),
    "n = 0": lambda: tuple(np.zeros(0, np.float32) for _ in range(3)),
    "cells at the grid's corners": _corners,
}

STATS = ["normals_neighbors", "normals_queries", "normals_tiles_small", "normals_tiles_sparse", "normals_tiles_dense",
         "normals_wide"]


@functools.lru_cache(maxsize=None)
def _cloud_and_reference(name):
    xyz = CLOUDS[name]()
    ref = O.normals(*xyz, E.R) if len(xyz[0]) else tuple(np.zeros(0, np.float32) for _ in range(4))
    return xyz, ref


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(CLOUDS))
def test_tiles_from_sorted_positions(monkeypatch, name):
    xyz, ref = _cloud_and_reference(name)
    n = len(xyz[0])
    seen = {}
    for mode in ("cells", "scan"):
        monkeypatch.setenv("PFX_LIST_SETUP", mode)
        with Context(0) as c:
            outs = [c.normals(*xyz, E.R), c.normals(*xyz, E.R)]  # the exact path, then a deferred build
            seen[mode] = {k: c.stat(k) for k in STATS} if n else {}  # (an empty cloud builds nothing: no statistics)
            finite = int(np.isfinite(np.stack(xyz)).all(axis=0).sum())
            if finite:
                assert c.stat("normals_setup_" + mode) >= 2
                assert c.stat("normals_queries") == finite
        for out in outs:
            for a, b in zip(out, ref):
                assert len(a) == n
                assert np.array_equal(_bits(a), _bits(b)), f"{name}: {mode} set-up vs oracle"
    print(name, seen["cells"])
    assert seen["cells"] == seen["scan"]


def test_layouts_are_what_the_names_say():
    """The blobs' sorted positions, recomputed from the cells (no GPU needed for this part)."""
    def starts(xyz):
        c = E.cells(np.stack(xyz, axis=1))
        dims = c.max(axis=0) + 1
        key = np.sort((c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2])
        return np.flatnonzero(np.r_[True, key[1:] != key[:-1]]), len(key)

    s, n = starts(_cloud_and_reference("start on the last position of a slice")[0])
    assert list(s) == [0, 1, P - 1]
    s, n = starts(_cloud_and_reference("start on the first position of a slice")[0])
    assert list(s) == [0, 1, P]
    s, n = starts(_cloud_and_reference("finite count a multiple of P")[0])
    assert n == P and list(s) == [0, 1, 1501]
    s, n = starts(_cloud_and_reference("a slice without a start")[0])
    assert list(s) == [0, 1, 101, 9101] and not ((s >= P) & (s < 2 * P)).any() and 9000 > 2 * P
    s, n = starts(_cloud_and_reference("most positions a start")[0])
    assert len(s) > 0.75 * n and n > 2 * P
    s, n = starts(_cloud_and_reference("every position a start")[0])
    assert len(s) == n and n > P


def test_overlapped_pipeline_is_the_same_with_the_gather_forked_or_in_line(monkeypatch):
    import torch
    from pcl_feature_extraction_amd.pipeline import OverlappedNarfFpfh, alloc
    from pcl_feature_extraction_amd.synth import synth_room
    n = 50_000
    x, y, z, _ = synth_room(n, 5)
    dev = torch.device("cuda", 0)
    b = alloc(torch, n, dev, max_keypoints=4096)
    b.x.copy_(torch.from_numpy(x)); b.y.copy_(torch.from_numpy(y)); b.z.copy_(torch.from_numpy(z))
    monkeypatch.setenv("PFX_GRID_BUILD", "sort")  # (a cloud this small would take the counting builder: no gather)
    outs = {}
    for fork in ("1", "0"):
        monkeypatch.setenv("PFX_GATHER_FORK", fork)
        ctx, ctx_n = Context(0), Context(0)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        run = OverlappedNarfFpfh(torch, ctx, ctx_n, dev)
        for call in range(2):  # the first call builds on exact bounds, the second on the hint
            reruns = ctx_n.stat("normals_speculative_reruns") if call else 0
            for t in (b.nx, b.ny, b.nz, b.curv, b.desc):
                t.fill_(-1.0)
            kp, k = run(b)
            torch.cuda.synchronize(dev)
            outs[fork, call] = (np.asarray(kp), *[t.cpu().numpy().view(np.uint32) for t in (b.nx, b.ny, b.nz, b.curv)],
                                b.desc[:k].cpu().numpy().view(np.uint32))
        assert ctx_n.stat("normals_speculative_reruns") == reruns, "the second call was redone"
        assert (ctx_n.stat("normals_gather_forked") > 0) == (fork == "1")
        run.close(); ctx.close(); ctx_n.close()
    assert len(outs["1", 0][0]) > 0
    for key in outs:
        for a, c in zip(outs[key], outs["1", 0]):
            assert np.array_equal(a, c), f"fork {key[0]}, call {key[1]}"
