"""The descriptors, keypoint detectors and ICP on grids whose cell is coarser than the search radius
(coarse_grid_cases.py; the grid itself, normals, radius_search, FPFH and SHOT-352:
test_gpu_coarse_grid.py).  Each operation goes through the comparison its own GPU test makes,
imported from there: raw bits and statistics against its CPU restatement.

Covered: SHOT-1344, PFH, spin images, the intensity gradient and RIFT, intensity spin, 3DSC and USC,
moment invariants and principal curvatures, BOARD, boundary points, CVFH (its filtered cloud keeps
the stray, so its normals' and its clustering's grids coarsen), Harris3D and Harris6D with refinement
(r = 0.01 on two_parts and on stray(3000), both scaled by 0.2), ICP with a distance cap against
stray, stray_near and two_parts targets.

Queries: cloud rows with a normal (so not the stray) and the point 0.6 r outside the box; PFH and the
moments, whose tests have rows without neighbours, also take the points a coarse cell and more
outside (coarse_grid_cases.queries).

Left out, because their grids cannot coarsen on clouds of this size:
  * knn_search and normals_knn: the cell comes from the bounding volume and the point count
    (pfx_knn.hip first_cell: 1.3 times the radius of the ball expected to hold k points), so on the
    cubic box a stray makes the grid has about (pi n / 6 k)^1.5 / 2.2 cells, 2^26 only beyond
    n / k = 530,000; later rounds double the cell;
  * cloud_resolution's own grid (pfx_iss.hip): its cell is 0.5 cbrt(volume / n) whatever the radius,
    8 n cells at the most.

Not covered: ISS on stray.  Its salient and non-maximum grids do coarsen when the radii come from the
patch's resolution (one stray adds 865 m / (n + 1) to the mean that the resolution is, so radii taken
from the stray cloud's own resolution are metres wide).  A test of both, test_gpu_iss.py's
_check_cloud on stray(3000) followed by iss_keypoints at 6 and 4 times the patch's resolution, did
not finish within seven minutes on the MI355X (every test of this file takes under two seconds).
Where it stood is not known: the run's output ends with the test before it, so the stall may have
been in a kernel of pfx_iss.hip, in the list build behind it or in the CPU oracle (both calls of the
oracle take about a second on a CPU-only machine).  _check_cloud takes its radii from the stray
cloud's own resolution, 6 x 0.298 m: every patch point then has all 3,000 points as neighbours, all
of them miss k_iss_cov's exactness bound (a coordinate of exactly 0 is among them), overflow
k_iss_ordered's 512 and go through masked neighbour lists of 3,000 entries each.  Reading k_nn2,
k_nn2_brute, k_iss_cov, k_iss_ordered, the host loops and build_lists' retry loop showed no
unbounded loop, so the cause is open and the test is not part of this file.
"""
import functools

import numpy as np
import pytest

import board_ref
import boundary_ref
import coarse_grid_cases as C
import cvfh_ref
import icp_ref
import intensity_spin_ref
import moments_ref
import oracle_lib as O
import pfh_ref
import rift_ref
import shape_context_ref
import shot_color_ref
import spin_ref
import test_gpu_board as TB
import test_gpu_boundary as TBD
import test_gpu_cvfh as TC
import test_gpu_harris as TH
import test_gpu_harris6d as TH6
import test_gpu_icp as TICP
import test_gpu_intensity_spin as TIS
import test_gpu_moments as TM
import test_gpu_pfh as TP
import test_gpu_rift as TR
import test_gpu_shape_context as TSC
import test_gpu_shot_color as TS
import test_gpu_spin as TSP
from pcl_feature_extraction_amd.synth import texture_rgb

pytestmark = pytest.mark.gpu

CASES = {
    "stray(3000)": lambda: C.stray(3000),
    "stray(12000)": lambda: C.stray(12000),
    "stray_near(12000)": lambda: C.stray_near(12000),
    "two_parts": lambda: C.two_parts(),
}
NAMES = list(CASES)
R_OF = {"stray(3000)": C.R_FEATURE, "stray(12000)": C.R, "stray_near(12000)": C.R, "two_parts": C.R}
REFS = {"pfh": pfh_ref, "spin": spin_ref, "rift": rift_ref, "ispin": intensity_spin_ref, "sc": shape_context_ref,
        "moments": moments_ref, "board": board_ref, "boundary": boundary_ref, "cvfh": cvfh_ref, "shot_color": shot_color_ref,
        "icp": icp_ref}


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """The restatements, each compiled when first asked for."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = REFS[name].build(tmp_path_factory.mktemp(name + "_ref"))
        return built[name]
    return get


@functools.lru_cache(maxsize=None)
def _case(name, off=1):
    """cloud, oracle normals + curvature at 0.05, intensities, colours; queries (cloud rows with a
    normal, then the first `off` off-cloud points), their normals, intensities' rows and colours."""
    xyz = CASES[name]()
    r = R_OF[name]
    assert C.factor(xyz, r) > 1.4
    nrm = O.normals(*xyz, C.R)
    (qx, qy, qz), rows = C.queries(xyz, r)
    on = np.flatnonzero((rows >= 0) & np.isfinite(nrm[0][np.maximum(rows, 0)]))
    keep = np.r_[on, np.flatnonzero(rows < 0)[:off]]
    q = tuple(np.ascontiguousarray(a[keep]) for a in (qx, qy, qz))
    src = np.where(rows[keep] >= 0, rows[keep], rows[on[0]])  # (an off-cloud query borrows a cloud row's normal)
    qn = tuple(np.ascontiguousarray(a[src]) for a in nrm[:3])
    x, y, z = (np.nan_to_num(a.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) for a in xyz)
    inten = (0.5 + 0.4 * np.sin(9.0 * x) * np.cos(7.0 * y) + 0.1 * np.sin(23.0 * z)).astype(np.float32)
    rgb = texture_rgb(*xyz, 3).astype(np.uint32)
    assert len(q[0]) >= 40 and np.isfinite(np.stack(qn)).all()
    return dict(xyz=xyz, r=r, nrm=nrm[:3], curv=nrm[3], q=q, qn=qn, inten=inten, rgb=rgb, qrgb=np.ascontiguousarray(rgb[src]))


@pytest.mark.parametrize("name", NAMES)
def test_shot_color(ctx, refs, name):
    c = _case(name)
    desc, want = TS.check(ctx, refs("shot_color"), c["xyz"], c["nrm"], c["rgb"], c["q"], c["qrgb"], c["r"])
    assert (~np.isnan(desc).any(axis=1)).sum() >= 5


@pytest.mark.parametrize("name", NAMES)
def test_pfh(ctx, refs, name):
    c = _case(name, off=6)
    got = TP.check(ctx, refs("pfh"), c["xyz"], c["nrm"], c["q"], c["r"])
    assert np.isnan(got[-5:]).all()  # no neighbour: no row


@pytest.mark.parametrize("name", NAMES)
def test_spin_image(ctx, refs, name):
    c = _case(name)
    TSP.check(ctx, refs("spin"), c["xyz"], c["q"], c["qn"], c["r"])


@pytest.mark.parametrize("name", NAMES)
def test_intensity_gradient_and_rift(ctx, refs, name):
    c = _case(name)
    xyz, r = c["xyz"], c["r"]
    TR.check_gradient(ctx, refs("rift"), xyz, c["inten"], c["q"], c["qn"], r)
    # the gradient at every point (the same_as_surface form), then RIFT on it
    want = TR.check_gradient(ctx, refs("rift"), xyz, c["inten"], xyz, c["nrm"], C.R, same_as_surface=True)
    grads = tuple(np.ascontiguousarray(want.out[:, i]) for i in range(3))
    TR.check_rift(ctx, refs("rift"), xyz, grads, c["q"], r)


@pytest.mark.parametrize("name", NAMES)
def test_intensity_spin(ctx, refs, name):
    c = _case(name)
    TIS.check(ctx, refs("ispin"), c["xyz"], c["inten"], c["q"], c["r"])


@pytest.mark.parametrize("name", NAMES)
def test_shape_context_and_usc(ctx, refs, name):
    c = _case(name)
    TSC.check_sc(ctx, refs("sc"), c["xyz"], c["nrm"], c["q"], c["r"])
    frames = ctx.shot_lrf(*c["xyz"], *c["q"], c["r"])
    TSC.check_usc(ctx, refs("sc"), c["xyz"], c["q"], frames, c["r"])


@pytest.mark.parametrize("name", NAMES)
def test_moments_and_principal_curvatures(ctx, refs, name):
    c = _case(name, off=6)
    ref = refs("moments")
    ctx.moment_invariants(*c["xyz"], *c["q"], c["r"])  # (the capacity statistic exists after a call)
    want = moments_ref.moments(ref, *c["xyz"], *c["q"], c["r"])
    TM.check_moments(ctx, ref, c["xyz"], c["q"], c["r"], queued_rows=TM.queued(ctx, want))
    want = moments_ref.curvatures(ref, *c["xyz"], *c["nrm"], *c["q"], *c["qn"], c["r"])
    TM.check_curvatures(ctx, ref, c["xyz"], c["nrm"], c["q"], c["qn"], c["r"], queued_rows=TM.queued(ctx, want))


@pytest.mark.parametrize("name", NAMES)
def test_board(ctx, refs, name):
    c = _case(name)
    ref = refs("board")
    want = board_ref.frames(ref, *c["xyz"], *c["nrm"], *c["q"], c["r"])
    ctx.board_lrf(*c["xyz"], *c["nrm"], *c["q"], c["r"])  # (the capacity statistic exists after a call)
    queued = int((want.k > ctx.stat("board_cap_small")).sum())
    TB.check(ctx, ref, c["xyz"], c["nrm"], c["q"], c["r"], queued_rows=queued)


@pytest.mark.parametrize("name", NAMES)
def test_boundary(ctx, refs, name):
    c = _case(name)
    want = TBD.check(ctx, refs("boundary"), c["xyz"], c["q"], c["qn"], c["r"])
    print(name, "boundary rows flagged", want.flagged, "of", len(c["q"][0]))


@pytest.mark.parametrize("name", ["stray(3000)", "two_parts"])
def test_cvfh(ctx, refs, name):
    """The stray is given a normal and a flat curvature, so it passes CVFH's curvature filter and
    stays in the filtered cloud: that cloud's normals (radius_normals) and its clustering
    (cluster_tolerance) then run on coarse grids."""
    c = _case(name)
    nx, ny, nz = (a.copy() for a in c["nrm"])
    curv = c["curv"].copy()
    if name != "two_parts":
        nx[-1], ny[-1], nz[-1], curv[-1] = 0.0, 0.0, 1.0, 0.0
    prm = cvfh_ref.params(radius_normals=C.R, cluster_tolerance=C.R, min_points=50)
    want = TC.check(ctx, refs("cvfh"), c["xyz"] + (nx, ny, nz, curv), prm=prm)
    print(name, want.stats)
    assert want.stats["cvfh_clusters"] >= 1
    if name != "two_parts":
        assert want.stats["cvfh_filtered"] > 1000 and want.labels[-1] == -1  # filtered in, too small for a cluster


# ---- keypoints --------------------------------------------------------------------------------------

def _scaled(xyz, s):
    return tuple((a * np.float32(s)).astype(np.float32) for a in xyz)


HARRIS = {"two_parts": lambda: C.two_parts(scale=C.HARRIS_SCALE),
          "stray(3000)": lambda: _scaled(C.stray(3000), C.HARRIS_SCALE)}


@pytest.mark.parametrize("name", list(HARRIS))
def test_harris3d_and_6d_with_refinement(ctx, name):
    xyz = HARRIS[name]()
    assert C.factor(xyz, C.R_HARRIS) > 1.4
    k, nc = TH._check(ctx, *xyz, refine=True, radius=C.R_HARRIS)
    print(name, "harris3d keypoints", k, "corners", nc)
    assert k > 0
    rgb = texture_rgb(*(a / np.float32(C.HARRIS_SCALE) for a in xyz), 5)
    k, nc = TH6._check(ctx, *xyz, rgb, refine=True, radius=C.R_HARRIS)
    print(name, "harris6d keypoints", k, "corners", nc)
    assert k > 0


# ---- ICP ---------------------------------------------------------------------------------------------

ICP_CASES = [("stray(3000)", 0.07), ("stray(3000)", 0.05), ("stray_near(12000)", 0.07), ("two_parts", 0.05),
             ("two_parts", 0.07)]


@pytest.mark.parametrize("name,cap", ICP_CASES)
def test_icp_with_a_distance_cap(ctx, refs, name, cap):
    """ICP's first cell, 0.5 cbrt(volume / n) of the target, is metres wide on these targets; the
    first level at or above the distance cap is cut down to cap (1 + 1e-4) (pfx_icp.hip), here
    level 0, and that grid and the doubled ones after it coarsen on the target's box.  The source
    is a third of the target moved by 3 cm (the stray's image pairs with the stray), a point outside
    the box within the cap, one beyond the cap inside the first coarse cell, a clamped one and a
    NaN (coarse_grid_cases.icp_source).  test_gpu_icp.py's comparison: every output's bits."""
    target = CASES[name]()
    lo, hi = C.bounds(target)
    ext = hi - lo
    h0 = 0.5 * np.cbrt(np.prod(np.maximum(ext, ext.max() * 1e-3)) / len(target[0]))
    cap_cell = cap * (1.0 + 1e-4)
    assert h0 >= cap_cell                                   # level 0 is the one cut down to the cap
    cells = [C.grid_params(lo, hi, cap_cell * 2 ** k)[0] / (cap_cell * 2 ** k) for k in range(4)]
    assert cells[0] > 1.05 and (name != "stray(3000)" or min(cells) > 1.4)  # (there all four levels coarsen)
    source = C.icp_source(target, cap)
    got, want = TICP.check(ctx, refs("icp"), (source, target, dict(max_correspondence_distance=cap), None))
    print(name, cap, "cell / asked cell per level", cells, "iterations", want.iterations, "pairs", want.n_last,
          "nn rounds", ctx.stat("icp_nn_rounds"), "brute", ctx.stat("icp_brute"))
    assert want.converged and want.n_last >= len(source[0]) - 4
