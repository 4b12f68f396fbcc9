"""GPU parity: the kernels that walk the normal estimation's neighbour lists with one lane per list
(k_harris_response, k_harris_nms, k_intensity_gradient, k_harris6d_response and k_igrad_lists;
DESIGN.md 15.2), on one small cloud built to sit on the edges of that walk.

Bar: bit-exact against the restatements the detectors' own suites use (oracle_lib for Harris3D and
Harris6D, rift_ref for the whole-cloud intensity gradient).

k_iss_scatter (pfx_iss.hip) keeps its own copy of the walk and is not run here; test_gpu_iss.py's
test_dense_cluster_at_origin_takes_the_list_path runs it.

The cloud (radius R, so grid cells of R from the bounding box's minimum, which is the origin):
tight blobs (0.02 R across, at least 2.5 R from everything else) whose points therefore have exactly
the blob's size as neighbourhood -- 1, 2, 3, 7, 8, 9, 16 and 17 points on a cell corner, so each
neighbourhood spreads over several cells and runs; 2, 3 and 20 points in the middle of a cell, so
those cells hold 2, 3 and 16-plus queries (lists interleaved at strides 2, 4 and 16); 7 points in
an edge cell and one point in the corner cell of the grid (clipped runs); a wavy sheet with
neighbourhoods around 20; two points with a NaN coordinate.  257 finite points: the second
workgroup of every kernel runs with one live lane.  The sizes are asserted below from
radius_search and grid_debug, so the cloud cannot silently stop covering them."""
import numpy as np
import pytest

import oracle_lib as O
import rift_ref as P
from parity import bits

pytestmark = pytest.mark.gpu

R = 0.05
SIZES = (1, 2, 3, 7, 8, 9, 16, 17)


def _blob(rng, centre_in_cells, m):
    return np.asarray(centre_in_cells, np.float64) * R + (rng.random((m, 3)) - 0.5) * (0.02 * R)


def _cloud():
    rng = np.random.default_rng(5)
    parts = [np.zeros((1, 3))]                                             # the corner cell (and the grid's origin)
    corners = [(3, 3, 3), (6, 3, 3), (9, 3, 3), (3, 6, 3), (6, 6, 3), (9, 6, 3), (3, 9, 3), (6, 9, 3)]
    parts += [_blob(rng, c, m) for c, m in zip(corners, SIZES)]            # across cells
    parts += [_blob(rng, (12.5, 3.5 + 3 * i, 3.5), m) for i, m in enumerate((2, 3, 20))]  # inside one cell
    parts.append(_blob(rng, (0.5, 6, 3), 7))                               # an edge cell (ix = 0)
    m = 257 - sum(len(p) for p in parts)
    u, v = rng.random((2, m))
    sheet = np.stack([3 + 6 * u, 11.5 + 4 * v, 3 + 0.3 * np.sin(5 * u) * np.cos(4 * v)], 1) * R
    parts.append(sheet + rng.normal(0, 0.01 * R, sheet.shape))
    pts = np.concatenate(parts).astype(np.float32)
    assert len(pts) == 257 and pts.min() == 0.0
    bad = np.array([[np.nan, 0.2, 0.1], [0.3, 0.3, np.nan]], np.float32)
    pts = np.concatenate([pts, bad])[rng.permutation(259)]
    rgb = rng.integers(0, 1 << 24, len(pts)).astype(np.uint32)
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy(), rgb


@pytest.fixture(scope="module")
def scene(ctx):
    x, y, z, rgb = _cloud()
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    assert fin.sum() == 257 and len(x) == 259
    counts, _, _ = ctx.radius_search(x, y, z, x, y, z, R)
    assert set(SIZES) <= set(counts[fin].tolist()), sorted(set(counts[fin].tolist()))
    assert (counts[~fin] == 0).all()
    g = ctx.grid_debug(x, y, z, R)
    per_cell = np.diff(g["cell_start"][: g["ncells"] + 1])
    assert {2, 3} <= set(per_cell.tolist()) and per_cell.max() >= 16, sorted(set(per_cell.tolist()))
    key = np.flatnonzero(per_cell)
    ix, iy = key // (g["nz"] * g["ny"]), (key // g["nz"]) % g["ny"]
    x_edge, y_edge = (ix == 0) | (ix == g["nx"] - 1), (iy == 0) | (iy == g["ny"] - 1)
    assert g["nx"] > 2 and g["ny"] > 2 and (x_edge & y_edge).any() and (x_edge ^ y_edge).any()
    return x, y, z, rgb


def _same(got, want, what, nan_bits=False):
    """Equal bits; a NaN's own bits count only where the restatement pins them (nan_bits), as in
    the detectors' suites."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not nan_bits:
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        got, want = np.nan_to_num(got, nan=-7.0), np.nan_to_num(want, nan=-7.0)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))
    assert len(bad) == 0, f"{what}: rows {bad[:8].tolist()} of {len(got)} differ"


def test_harris3d_response(ctx, scene):
    x, y, z, _ = scene
    kp_o, resp_o, cor_o = O.harris3d(x, y, z, R, 1e-6, True)
    kp_g, resp_g, cor_g = ctx.harris3d_keypoints(x, y, z, R, 1e-6, True, details=True)
    _same(resp_g, resp_o, "response")
    _same(cor_g, cor_o, "corners")
    assert np.array_equal(kp_g, kp_o)
    assert np.count_nonzero(resp_o) > 100


def test_harris6d_gradient_and_response(ctx, scene):
    x, y, z, rgb = scene
    kp_o, resp_o, cor_o, g_o = O.harris6d(x, y, z, rgb, R, 1e-6, True)
    kp_g, resp_g, cor_g, g_g = ctx.harris6d_keypoints(x, y, z, rgb, R, 1e-6, True, details=True)
    _same(g_g, g_o, "gradient")
    _same(resp_g, resp_o, "response")
    _same(cor_g, cor_o, "corners")
    assert np.array_equal(kp_g, kp_o)
    assert np.isnan(g_o).all(axis=1).sum() == 2 and np.count_nonzero(np.nan_to_num(g_o)) > 100


def test_whole_cloud_intensity_gradient(ctx, scene, tmp_path_factory):
    from pcl_feature_extraction_amd import rgb_to_intensity
    x, y, z, rgb = scene
    ref = P.build(tmp_path_factory.mktemp("rift_ref"))
    inten = rgb_to_intensity(rgb)
    inten[[11, 140]] = np.nan, np.inf  # neighbours the second pass leaves out
    nrm = tuple(ctx.normals(x, y, z, R)[:3])
    want = P.gradient(ref, x, y, z, inten, x, y, z, *nrm, R)
    got = ctx.intensity_gradient(x, y, z, inten, x, y, z, *nrm, R, same_as_surface=True)
    _same(got, want.out, "whole-cloud gradient", nan_bits=True)
    assert (ctx.stat("igrad_neighbors"), ctx.stat("igrad_kmax")) == (want.neighbors, want.kmax)
    assert np.isfinite(want.out).all(axis=1).sum() > 100

