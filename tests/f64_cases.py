"""Seeded small clouds for the float64 statements (tests/f64_ref.py), each with a check of its own
non-vacuity made when it is built -- TEST INFRASTRUCTURE ONLY.

Every case is float32 data as the product gets it.  A case function raises if one of its checks
fails (a new seed is the remedy, never a looser check):
  * no (centre, point) pair lies within a relative RADIUS_MARGIN of r^2 at any radius the case is
    used with, so a float32 and a float64 radius search return the same sets;
  * rough_blob*: at least 30 of the 33 FPFH bins hold more than 1 % in every finite row;
  * aniso_blob: at least 100 non-zero SHOT bins in every finite row;
  * aniso_blob, dense_core: every frame has a relative eigen-gap of SHOT_GAP_CASE at the least
    and no tied sign vote (the comparison itself leaves out only gaps below a tenth of that);
  * dense_core: the dense query has more than 2,048 neighbours, no other query has.
The float64 results the checks need are kept on the case (`ref`), so a test does not pay twice.
"""
import functools
from types import SimpleNamespace

import numpy as np

import f64_ref as R

RADIUS_MARGIN = 1e-5
TAU = 1e-4                  # FPFH: width of the ambiguous band around a bin edge, in bins
SPLIT_CAPACITY = 2048       # SHOT: lists longer than this leave the split kernels (kCapSmall)
SHOT_GAP_CASE = 1e-2        # SHOT: smallest relative eigen-gap of a frame in a case


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _require(ok, what):
    if not ok:
        raise AssertionError("f64 case is vacuous, pick another seed: " + what)


def _require_margin(name, P, Q, r):
    m = R.radius_margin(P, Q, r)
    _require(m > RADIUS_MARGIN, "%s: a pair at %.3g of r^2 (r = %g)" % (name, m, r))


def _fpfh_case(name, P, N, Q, r):
    _require_margin(name, P, P, r)
    _require_margin(name, P, Q, r)
    lo, hi, share = R.fpfh_interval(P, N, Q, r, False, TAU)
    fin = np.isfinite(lo).all(1)
    _require(fin.sum() >= 20, "%s: %d finite rows" % (name, fin.sum()))
    filled = (lo[fin] > 1.0).sum(1)
    _require(filled.min() >= 30, "%s: a row with %d bins above 1 %%" % (name, filled.min()))
    return SimpleNamespace(name=name, P=P, N=N, Q=Q, r=r, ref=SimpleNamespace(lo=lo, hi=hi, share=share))


def _blob(seed):
    rng = np.random.default_rng(seed)
    P = (np.array([0.3, -0.2, 1.1]) + rng.uniform(-0.06, 0.06, (1200, 3))).astype(np.float32)
    return rng, P, _unit(rng, 1200).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rough_blob(seed=2):
    """1,200 points uniform in a 0.12 m cube with independent random unit normals, r = 0.03
    (k ~ 55), every 60th point a query: FPFH with every bin of every block populated (on a smooth
    surface all mass sits in the middle bin of each block and a comparison proves nothing)."""
    _, P, N = _blob(seed)
    return _fpfh_case("rough_blob", P, N, P[::60].copy(), 0.03)


@functools.lru_cache(maxsize=None)
def rough_blob_keypoints(seed=2):
    """rough_blob's cloud with 25 queries that are not cloud points, one far away and one NaN:
    FPFH's keypoints != surface branch and its NaN rows."""
    rng, P, N = _blob(seed)
    Q = (np.array([0.3, -0.2, 1.1]) + rng.uniform(-0.05, 0.05, (25, 3))).astype(np.float32)
    Q = np.concatenate([Q, np.array([[10.0, 10.0, 10.0], [np.nan, 0.0, 0.0]], np.float32)])
    c = _fpfh_case("rough_blob_keypoints", P, N, Q, 0.03)
    _require(np.isnan(c.ref.lo[-2:]).all() and np.isfinite(c.ref.lo[:-2]).all(), "rough_blob_keypoints: NaN rows")
    return c


def shot_reference(P, N, Q, r):
    frames = [R.shot_lrf(P, q, r) for q in Q]
    rf = np.array([f[0] for f in frames])
    cond = np.array([f[1] for f in frames], np.float64)
    desc = np.array([R.shot352(P, N, q, f, r) for q, f in zip(Q, rf)])
    return SimpleNamespace(rf=rf, cond=cond, desc=desc)


def _require_conditioned(name, ref):
    """The comparison leaves out frames with a relative eigen-gap below 1e-3 or a tied sign vote;
    between that and a well separated frame a rounding error is merely amplified by 1 / gap.  The
    cases are to measure arithmetic, so their frames keep ten times that distance."""
    fin = np.isfinite(ref.rf).all(1)
    _require(ref.cond[fin, 0].min() >= SHOT_GAP_CASE, "%s: a frame with relative eigen-gap %.3g"
             % (name, ref.cond[fin, 0].min()))
    _require(ref.cond[fin, 1:].min() >= 1, name + ": a tied sign vote")


def _aniso(seed):
    rng = np.random.default_rng(seed)
    P = rng.normal(0.0, (0.05, 0.035, 0.02), (1500, 3)).astype(np.float32)
    return rng, P, _unit(rng, 1500).astype(np.float32)


@functools.lru_cache(maxsize=None)
def aniso_blob(seed=119):
    """1,500 points normal(0, (0.05, 0.035, 0.02)) with random unit normals, r = 0.04, every 50th
    point a query: the SHOT frame and descriptor."""
    _, P, N = _aniso(seed)
    Q, r = P[::50].copy(), 0.04
    _require_margin("aniso_blob", P, Q, r)
    ref = shot_reference(P, N, Q, r)
    fin = np.isfinite(ref.desc).all(1)
    _require(fin.sum() >= 20, "aniso_blob: %d finite rows" % fin.sum())
    filled = (ref.desc[fin] != 0).sum(1)
    _require(filled.min() >= 100, "aniso_blob: a row with %d non-zero bins" % filled.min())
    _require_conditioned("aniso_blob", ref)
    return SimpleNamespace(name="aniso_blob", P=P, N=N, Q=Q, r=r, ref=ref)


@functools.lru_cache(maxsize=None)
def dense_core(seed=119):
    """aniso_blob plus 2,200 points within r/2 of its first query, which then has more than 2,048
    neighbours: SHOT's fused long-list kernel next to the split kernels.  `dense` is that row."""
    rng, P, N = _aniso(seed)
    Q, r = P[::50].copy(), 0.04
    v = _unit(rng, 2200) * (0.5 * r * rng.uniform(0.0, 1.0, (2200, 1)) ** (1.0 / 3.0))
    P = np.concatenate([P, (Q[0].astype(np.float64) + v).astype(np.float32)])
    N = np.concatenate([N, _unit(rng, 2200).astype(np.float32)])
    _require_margin("dense_core", P, Q, r)
    ref = shot_reference(P, N, Q, r)
    k = np.array([len(R.neighbours(P, q, r)[0]) for q in Q])
    _require(k[0] > SPLIT_CAPACITY, "dense_core: dense query has k = %d" % k[0])
    _require((k[1:] <= SPLIT_CAPACITY).all(), "dense_core: a second long list")
    _require_conditioned("dense_core", ref)
    return SimpleNamespace(name="dense_core", P=P, N=N, Q=Q, r=r, ref=ref, k=k, dense=0)


def _patch(seed):
    """2,000 points of a bumpy 0.5 m x 0.2 m surface patch centred on the origin, in float64: an
    80 x 25 grid with every point moved by up to 0.3 of the spacing.  (Points drawn independently
    come arbitrarily close to each other, and a neighbour at a tenth of the usual distance takes
    nearly all of a point's 1 / d^2 weight: one ambiguous pair in that neighbour's SPFH is then more
    than 1 % of the row, whatever the radius.)"""
    rng = np.random.default_rng(seed)
    gu, gv = np.meshgrid((np.arange(80) + 0.5) / 80.0 - 0.5, (np.arange(25) + 0.5) / 25.0 - 0.5, indexing="ij")
    u = 0.5 * (gu.ravel() + rng.uniform(-0.3, 0.3, 2000) / 80.0)
    v = 0.2 * (gv.ravel() + rng.uniform(-0.3, 0.3, 2000) / 25.0)
    z = 0.008 * np.sin(31.0 * u) * np.cos(23.0 * v) + 0.004 * np.sin(67.0 * v + 1.0) + rng.normal(0.0, 0.0007, 2000)
    return np.stack([u, v, z], 1)[rng.permutation(2000)]   # (no grid order in the indices)


def _normals_case(name, P, vp, r=0.03):
    _require_margin(name, P, P, r)
    ref = R.normals(P, r, vp)
    _require(np.isfinite(ref.n).all(), name + ": a point with fewer than 3 neighbours")
    return SimpleNamespace(name=name, P=P, r=r, viewpoint=vp, ref=ref)


@functools.lru_cache(maxsize=None)
def surface_origin(seed=117):
    """The patch at the origin, viewpoint (0, 0, 2), r = 0.03: normals where a float32 single-pass
    covariance loses nothing (|p|^2 is of the order of the covariance itself): the tight bound."""
    return _normals_case("surface_origin", _patch(seed).astype(np.float32), (0.0, 0.0, 2.0))


@functools.lru_cache(maxsize=None)
def surface_range(seed=117):
    """The same patch translated to (0.3, -0.2, 1.5), viewpoint at the origin: normals at working
    range, where the single-pass covariance's error scales with |p|^2."""
    P = (_patch(seed) + np.array([0.3, -0.2, 1.5])).astype(np.float32)
    return _normals_case("surface_range", P, (0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def surface_chain(seed=117):
    """surface_origin chained as the reference chains it: its normals (taken from the product under
    test) feed FPFH over the whole cloud (same_as_surface, r_fpfh = 0.06) and SHOT at every 50th
    point (r_shot = 0.12, wider than the patch, so the frames are far from degenerate)."""
    c = surface_origin(seed)
    q = np.arange(0, len(c.P), 50)
    _require_margin("surface_chain fpfh", c.P, c.P, 0.06)
    _require_margin("surface_chain shot", c.P, c.P[q], 0.12)
    return SimpleNamespace(name="surface_chain", P=c.P, r=c.r, viewpoint=c.viewpoint, ref=c.ref, r_fpfh=0.06,
                           r_shot=0.12, queries=q, Q=c.P[q].copy())
