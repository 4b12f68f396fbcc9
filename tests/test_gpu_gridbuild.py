"""The grid's counting-sort builder (pfx_grid.hip, speculative builds) and the list set-up from the
cells (pfx_nblist.hip k_tile_cells) against NumPy, the radix-sort builder and the scan set-up.

The grid reference is NumPy on the exact double parameters the hook returns (Context.grid_debug):
key = (ix * ny + iy) * nz + iz from floor((double(p) - lo) * inv), clamped; non-finite points -> C;
perm = stable argsort of the keys; cell_start by searchsorted.  Every comparison is of raw bytes.
"""
import numpy as np
import pytest

import list_edge_clouds as E
import oracle_lib as O
from pcl_feature_extraction_amd import Context

pytestmark = pytest.mark.gpu

R = 0.05
FAT_BIT = 1 << 30
ARRAYS = ("perm", "skeys", "cell_start", "sp")
PARAMS = ("ox", "oy", "oz", "inv", "nx", "ny", "nz", "ncells")


def _ref_grid(x, y, z, g):
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    n, C = len(x), g["ncells"]
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)

    def cell(p, lo, dim):
        return np.clip(np.floor((p[fin].astype(np.float64) - lo) * g["inv"]), 0, dim - 1).astype(np.int64)

    key = np.full(n, C, np.int64)
    key[fin] = (cell(x, g["ox"], g["nx"]) * g["ny"] + cell(y, g["oy"], g["ny"])) * g["nz"] + cell(z, g["oz"], g["nz"])
    perm = np.argsort(key, kind="stable")
    skeys = key[perm]
    return {"perm": perm.astype(np.int32), "skeys": skeys.astype(np.uint32),
            "cell_start": np.searchsorted(skeys, np.arange(C + 2), side="left").astype(np.int32),
            "sp": np.stack([x[perm], y[perm], z[perm], np.zeros(n, np.float32)], axis=1)}


def _same_arrays(a, b, what):
    for k in ARRAYS:
        assert a[k].shape == b[k].shape, f"{what}: {k} shape"
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _same_grid(a, b, what):
    assert [a[k] for k in PARAMS] == [b[k] for k in PARAMS], f"{what}: parameters"
    _same_arrays(a, b, what)


def _check(g, xyz, what):
    _same_arrays(g, _ref_grid(*xyz, g), what + " vs numpy")
    return g


def _hinted(c, xyz, monkeypatch, builder):
    monkeypatch.setenv("PFX_GRID_BUILD", builder)
    g = c.grid_debug(*xyz, R, mode=1)
    monkeypatch.delenv("PFX_GRID_BUILD")
    return g


def _exact_then_both(xyz, monkeypatch, what, repeats=1):
    """mode 0, then hinted counting builds and one hinted radix build on one context: all exact."""
    with Context(0) as c:
        g0 = _check(c.grid_debug(*xyz, R, mode=0), xyz, what + " exact")
        assert g0["builder"] == "sort" and not g0["rerun"]
        gs = _check(_hinted(c, xyz, monkeypatch, "sort"), xyz, what + " hinted sort")
        assert gs["builder"] == "sort" and gs["word"] == 0 and not gs["rerun"]
        counts = c.stat("grid_count_builds")
        for i in range(repeats):
            gc = _check(_hinted(c, xyz, monkeypatch, "count"), xyz, what + " hinted count")
            assert gc["builder"] == "count" and gc["word"] == 0 and not gc["rerun"]
            _same_grid(gc, gs, what + f" count build {i} vs radix build")
        assert c.stat("grid_count_builds") == counts + repeats
    return g0, gc


def test_uniform_shuffled_cloud_and_repeats(monkeypatch):
    p = np.random.default_rng(1).uniform(0, 1, (20_000, 3)).astype(np.float32)
    xyz = (p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy())
    _exact_then_both(xyz, monkeypatch, "uniform", repeats=3)


def test_non_finite_rows_keep_index_order(monkeypatch):
    n = 10_000
    rng = np.random.default_rng(2)
    t = np.arange(n) / n  # scan order: neighbours in index are neighbours in space
    p = np.stack([t, 0.5 + 0.3 * np.sin(40 * t), 0.2 * np.cos(13 * t)], axis=1).astype(np.float32)
    bad = np.flatnonzero(rng.uniform(size=n) < 0.3)
    p[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(bad))
    xyz = (p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy())
    _, g = _exact_then_both(xyz, monkeypatch, "non-finite")
    C = g["ncells"]
    assert g["cell_start"][C] == n - len(bad) and g["cell_start"][C + 1] == n
    assert np.array_equal(g["perm"][n - len(bad):], bad)
    assert (g["skeys"][n - len(bad):] == C).all()


def _with_duplicates(k, far=False, seed=3):
    """5,000 points in the unit cube, then k copies of one point ten cells beyond it (a cell of its
    own), then (far) one point outside any hint of the rest."""
    p = np.random.default_rng(seed).uniform(0, 1, (5_000, 3))
    parts = [p, np.repeat([[1.5, 0.5, 0.5]], k, axis=0)]
    if far:
        parts.append([[40.0, 0.5, 0.5]])
    p = np.concatenate(parts).astype(np.float32)
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def _exact_on_fresh_context(xyz):
    with Context(0) as c:
        return c.grid_debug(*xyz, R, mode=0)


def test_cell_at_the_cap_and_one_above(monkeypatch):
    with Context(0) as c:
        cap = c.grid_debug(*_with_duplicates(1), R, mode=0)["cap"]
    at, above = _with_duplicates(cap), _with_duplicates(cap + 1)
    with Context(0) as c:
        _check(c.grid_debug(*at, R, mode=0), at, "cap exact")
        g = _check(_hinted(c, at, monkeypatch, "count"), at, "cap count")
        assert g["builder"] == "count" and g["word"] == 0 and not g["rerun"]
        assert np.diff(g["cell_start"]).max() == cap
        _same_grid(g, _hinted(c, at, monkeypatch, "sort"), "cap: count vs radix")
        assert c.stat("grid_fat_fallbacks") == 0
        g = _check(c.grid_debug(*above, R, mode=1), above, "cap + 1")
        assert g["builder"] == "count" and g["word"] == FAT_BIT and g["rerun"]
        _same_grid(g, _exact_on_fresh_context(above), "cap + 1: what the caller ends up with vs radix")
        assert c.stat("grid_fat_fallbacks") == 1
        sorts = c.stat("grid_hinted_sort_builds")
        g = _check(c.grid_debug(*above, R, mode=1), above, "cap + 1 again")
        assert g["builder"] == "sort" and g["word"] == 0 and not g["rerun"]
        assert c.stat("grid_hinted_sort_builds") == sorts + 1 and c.stat("grid_fat_fallbacks") == 1


@pytest.mark.parametrize("case", ["one point", "all non-finite", "flat"])
def test_edge_clouds(monkeypatch, case):
    if case == "one point":
        p = np.array([[0.25, -1.0, 3.0]], np.float32)
    elif case == "all non-finite":
        p = np.full((300, 3), np.nan, np.float32)
        p[::3, 1] = np.inf
    else:
        p = np.random.default_rng(4).uniform(0, 1, (3_000, 3)).astype(np.float32)
        p[:, 2] = 0.3
    xyz = (p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy())
    g0, g = _exact_then_both(xyz, monkeypatch, case)
    if case == "flat":
        assert g0["nz"] == 1
    if case == "all non-finite":
        assert g["cell_start"][g["ncells"]] == 0 and np.array_equal(g["perm"], np.arange(len(p)))


def test_point_outside_the_hint_with_a_fat_cell():
    with Context(0) as c:
        cap = c.grid_debug(*_with_duplicates(1), R, mode=0)["cap"]
        both = _with_duplicates(cap + 1, far=True)
        g = _check(c.grid_debug(*both, R, mode=1), both, "outside + fat")
        assert g["builder"] == "count" and g["rerun"]
        assert g["word"] & FAT_BIT and (g["word"] & ~FAT_BIT) == 1  # the fat bit and one point outside
        _same_grid(g, _exact_on_fresh_context(both), "outside + fat: exact rerun")
        assert c.stat("grid_fat_fallbacks") == 1


SETUP_CLOUDS = {
    "tile edges": lambda: E.exact_k_blobs((16, 384, 512, 1024, 2048, 4096))[0],
    "candidate classes": lambda: E.two_blob_blocks([(100, 384), (100, 385), (100, 1280), (100, 1281), (100, 8000),
                                                    (100, 8001), (600, 1280)])[0],
    "ties": lambda: E.ties_cloud((513, 1025), (17, 385, 513, 1025))[0],
    "lattice": lambda: E.binary_lattice()[0],
    "one per cell": E.one_per_cell_lattice,
    "cells of 1, 15, 16, 17, 31, 32, 33": lambda: E.exact_k_blobs((16, 32))[0],
}

SETUP_STATS = ["normals_neighbors", "normals_queries", "normals_tiles_small", "normals_tiles_sparse",
               "normals_tiles_dense", "normals_wide"]


@pytest.mark.parametrize("name", list(SETUP_CLOUDS))
def test_tiles_from_cells_equal_the_scan_setup(monkeypatch, name):
    xyz = SETUP_CLOUDS[name]()
    r = E.LATTICE_R if name == "lattice" else E.R
    ref = O.normals(*xyz, r)
    seen = {}
    for mode in ("cells", "scan"):
        monkeypatch.setenv("PFX_LIST_SETUP", mode)
        with Context(0) as c:
            outs = [c.normals(*xyz, r), c.normals(*xyz, r)]  # the exact path, then a deferred build
            stats = {k: c.stat(k) for k in SETUP_STATS}
            assert c.stat("normals_setup_" + mode) >= 2
        for out in outs:
            for a, b in zip(out, ref):
                a, b = (np.ascontiguousarray(v, np.float32).view(np.uint32) for v in (a, b))
                assert np.array_equal(a, b), f"{name}: {mode} set-up vs oracle"
        seen[mode] = stats
    print(seen["cells"])
    assert seen["cells"] == seen["scan"]


def test_overlapped_pipeline_is_the_same_under_both_builders(monkeypatch):
    import torch
    from pcl_feature_extraction_amd.pipeline import OverlappedNarfFpfh, alloc
    from pcl_feature_extraction_amd.synth import synth_room
    n = 50_000
    x, y, z, _ = synth_room(n, 5)
    dev = torch.device("cuda", 0)
    b = alloc(torch, n, dev, max_keypoints=4096)
    b.x.copy_(torch.from_numpy(x)); b.y.copy_(torch.from_numpy(y)); b.z.copy_(torch.from_numpy(z))
    outs = {}
    for builder in ("sort", "count"):
        monkeypatch.setenv("PFX_GRID_BUILD", builder)
        ctx, ctx_n = Context(0), Context(0)
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        run = OverlappedNarfFpfh(torch, ctx, ctx_n, dev)
        for call in range(2):
            reruns = ctx_n.stat("normals_speculative_reruns") if call else 0
            counted = ctx.stat("grid_count_builds") + ctx_n.stat("grid_count_builds")
            for t in (b.nx, b.ny, b.nz, b.curv, b.desc):
                t.fill_(-1.0)
            kp, k = run(b)
            torch.cuda.synchronize(dev)
            outs[builder, call] = (np.asarray(kp), *[t.cpu().numpy().view(np.uint32) for t in (b.nx, b.ny, b.nz, b.curv)],
                                   b.desc[:k].cpu().numpy().view(np.uint32))
        moved = ctx.stat("grid_count_builds") + ctx_n.stat("grid_count_builds") - counted
        assert ctx_n.stat("normals_speculative_reruns") == reruns, "the second call was redone"
        assert (moved > 0) == (builder == "count")
        run.close(); ctx.close(); ctx_n.close()
    assert len(outs["sort", 0][0]) > 0
    for key in outs:
        for a, c in zip(outs[key], outs["sort", 0]):
            assert a.shape == c.shape and np.array_equal(a, c), key
