"""The comparisons of a product (the CPU restatement in tests/test_f64_ref.py, the HIP kernels in
tests/test_gpu_f64.py) with the float64 statements of tests/f64_ref.py, and their bounds -- TEST
INFRASTRUCTURE ONLY.  Both test files import the bounds from here; neither redefines one.

Where the bounds come from (DESIGN.md "Float64 statements of normals, FPFH and SHOT"):
  * normals: derived.  The product sums nine float32 moments one neighbour after the other; the
    worst case of that sum perturbs the covariance by |E| = 3 (k + 2) 2^-24 max|p|^2, and by
    Davis-Kahan the normal turns by at most 2 |E| / gap, the curvature moves by at most
    2 |E| / trace.
  * FPFH (S_FPFH) and SHOT (T_RF, T_DESC): the worst figure of the restatement against the
    statements on the cases of tests/f64_cases.py, times 8, rounded up to one significant digit.
    The project's bars, 1e-3 on a block sum and 1e-4 L2 per row, are ceilings: a bound may use a
    tenth of its ceiling at the most.
"""
from types import SimpleNamespace

import numpy as np

import f64_cases as C
import f64_ref as R

# measured on the CPU restatement (the worst case of tests/f64_cases.py)      measured   x 8
S_FPFH = 1e-4       # FPFH: slack on either side of the interval, 0-100 scale  6.15e-6    4.9e-5  (blobs)
#                     surface_chain, where one bin holds 90 of a block's 100:  7.8e-5     6.2e-4  capped, see below
T_RF = 2e-6         # SHOT: largest |rf - rf64| of a frame component           2.12e-7    1.7e-6
T_DESC = 2e-6       # SHOT: L2 of a descriptor row against float64             2.22e-7    1.8e-6
# S_FPFH is not 8 x the chain's figure: that would be 7e-4, and a bound may not use more than a tenth
# of the 1e-3 bar.  It is that tenth.  The chain's float32 sums of ~225 terms into a bin holding 90
# are off by ten ulp of the bin's value (7.6e-6 each), which leaves a margin of 1.3, not 8.

SHARE_MAX = 1.0               # FPFH: largest ambiguous share of a row, 1 % of a block
NORMALS_LEFT_OUT_MAX = 0.05   # normals: rows left out of the sign-sensitive comparison
SHOT_GAP_MIN = 1e-3           # SHOT: smallest relative eigen-gap of a compared frame
SHOT_LEFT_OUT_MAX = 0.10
SHARP = 0.90                  # a planted error fails on this share of the finite rows


def same_nan_rows(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"


def _angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))


def normals_figures(ref, got):
    """ref: f64_ref.Normals; got: (nx, ny, nz, curvature) float32.  Asserts the NaN pattern and
    the derived bounds; returns the figures (worst angle and curvature difference, each also as a
    share of its bound, and the share of rows left out)."""
    n = np.stack([np.asarray(a, np.float64) for a in got[:3]], 1)
    curv = np.asarray(got[3], np.float64)
    same_nan_rows(n, ref.n)
    same_nan_rows(curv, ref.curvature)
    fin = np.isfinite(ref.n).all(1)
    err = 3.0 * (ref.k + 2) * 2.0 ** -24 * ref.pmax2
    with np.errstate(invalid="ignore", divide="ignore"):
        angle_bound = 2.0 * err / ref.gap
        curv_bound = 2.0 * err / ref.trace
        separated = fin & (ref.gap >= 4.0 * err)
        signed = separated & (ref.facing >= angle_bound)
    left_out = 1.0 - signed.sum() / fin.sum()
    assert left_out <= NORMALS_LEFT_OUT_MAX, left_out
    unsigned_angle = _angle(n[separated], ref.n[separated])
    unsigned_angle = np.minimum(unsigned_angle, np.pi - unsigned_angle)
    assert (unsigned_angle <= angle_bound[separated]).all(), (unsigned_angle / angle_bound[separated]).max()
    angle = _angle(n[signed], ref.n[signed])
    assert (angle <= angle_bound[signed]).all(), (angle / angle_bound[signed]).max()
    dc = np.abs(curv[fin] - ref.curvature[fin])
    assert (dc <= curv_bound[fin]).all(), (dc / curv_bound[fin]).max()
    return dict(angle=angle.max(), angle_of_bound=(angle / angle_bound[signed]).max(), curvature=dc.max(),
                curvature_of_bound=(dc / curv_bound[fin]).max(), left_out=left_out, rows=int(fin.sum()))


def fpfh_excess(ref, got):
    """Per row, how far outside [lo, hi] the worst value of the row lies (0: inside); NaN for a NaN row."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        return np.maximum(np.maximum(ref.lo - got, got - ref.hi), 0.0).max(1)


def fpfh_figures(ref, got):
    same_nan_rows(got, ref.lo)
    fin = np.isfinite(ref.lo).all(1)
    assert fin.any()
    assert ref.share[fin].max() <= SHARE_MAX, ref.share[fin].max()
    ex = fpfh_excess(ref, got)[fin]
    assert ex.max() <= S_FPFH, ex.max()
    return dict(excess=ex.max(), share=ref.share[fin].max(), rows=int(fin.sum()))


def shot_compared_rows(ref):
    """The finite rows whose frame is well enough conditioned to be compared, after asserting that
    few enough are left out."""
    fin = np.isfinite(ref.rf).all(1)
    with np.errstate(invalid="ignore"):
        use = fin & (ref.cond[:, 0] >= SHOT_GAP_MIN) & (ref.cond[:, 1] > 0) & (ref.cond[:, 2] > 0)
    assert fin.any() and 1.0 - use.sum() / fin.sum() <= SHOT_LEFT_OUT_MAX, (use.sum(), fin.sum())
    return use


def shot_errors(ref, desc, rf):
    """Per row: (largest |rf - rf64|, L2 of desc - desc64)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(rf, np.float64) - ref.rf).max(1),
                np.linalg.norm(np.asarray(desc, np.float64) - ref.desc, axis=1))


def shot_figures(ref, desc, rf, desc_own_frame):
    """desc, rf: the product's; desc_own_frame: the float64 descriptor computed in the product's
    own float32 frame (frame error taken out: what is left is the histogram's)."""
    same_nan_rows(desc, ref.desc)
    same_nan_rows(rf, ref.rf)
    use = shot_compared_rows(ref)
    e_rf, e_desc = shot_errors(ref, desc, rf)
    e_hist = np.linalg.norm(np.asarray(desc, np.float64) - desc_own_frame, axis=1)
    assert e_rf[use].max() <= T_RF, e_rf[use].max()
    assert e_desc[use].max() <= T_DESC, e_desc[use].max()
    assert e_hist[use].max() <= T_DESC, e_hist[use].max()
    return dict(rf=e_rf[use].max(), desc=e_desc[use].max(), desc_own_frame=e_hist[use].max(), rows=int(use.sum()),
                gap=np.nanmin(ref.cond[use, 0]), margin=int(np.nanmin(ref.cond[use, 1:])))


# ---- the comparisons of section (a), for any product with the restatement's call forms --------
# (tests/oracle_lib.py and pcl_feature_extraction_amd.Context take the same positional arguments)

def xyz(a):
    a = np.asarray(a, np.float32)
    return [np.ascontiguousarray(a[:, i]) for i in range(3)]


def run_normals(product, case):
    got = product.normals(*xyz(case.P), case.r, case.viewpoint)
    return normals_figures(case.ref, got), got


def run_fpfh(product, case):
    got = product.fpfh(*xyz(case.P), *xyz(case.N), *xyz(case.Q), case.r, False)
    return fpfh_figures(case.ref, got), got


def shot_own_frame(case, rf, N=None, r=None):
    """The float64 descriptor of every query in the given (the product's float32) frames."""
    N = case.N if N is None else N
    return np.array([R.shot352(case.P, N, q, f, case.r if r is None else r) for q, f in zip(case.Q, rf)])


def run_shot(product, case):
    desc, rf = product.shot(*xyz(case.P), *xyz(case.N), *xyz(case.Q), case.r)
    return shot_figures(case.ref, desc, rf, shot_own_frame(case, rf)), (desc, rf)


def run_chain(product, case):
    """normals -> FPFH (same_as_surface) -> SHOT, every stage on the product's own output of the
    stage before it, every stage against the float64 statement of it on the same float32 input."""
    fig = {}
    fig["normals"], n = run_normals(product, case)
    N = np.stack([np.asarray(a, np.float32) for a in n[:3]], 1)
    got = product.fpfh(*xyz(case.P), *xyz(N), *xyz(case.P), case.r_fpfh, True)
    lo, hi, share = R.fpfh_interval(case.P, N, None, case.r_fpfh, True, C.TAU)
    fig["fpfh"] = fpfh_figures(SimpleNamespace(lo=lo, hi=hi, share=share), got)
    desc, rf = product.shot(*xyz(case.P), *xyz(N), *xyz(case.Q), case.r_shot)
    ref = C.shot_reference(case.P, N, case.Q, case.r_shot)
    fig["shot"] = shot_figures(ref, desc, rf, shot_own_frame(case, rf, N, case.r_shot))
    return fig, (n, got, desc, rf)
