"""Plain float64 statements of radius search, normal estimation, FPFH-33 and SHOT-352 -- TEST
INFRASTRUCTURE ONLY (numpy).

Written from SURVEY.md Appendix A (A.1, A.2, A.3, A.7) and the papers of PAPERS.md, in whatever
structure is natural in numpy: a two-pass covariance and LAPACK's eigh for the normals, an
interval-valued histogram for FPFH, an 8 x 2 x 2 x 11 tensor with multilinear weights for SHOT.
Nothing here calls into oracle/ or follows its float32 operation order: the inputs are the
float32 arrays the product gets, every operation on them is float64.

Each statement also returns the conditioning numbers a comparison needs to tell a rounding
difference from a wrong reading (an eigen-gap, a sign margin, the distance to a decision).

CONVENTIONS names the readings of the definitions that tests/test_f64_ref.py plants errors in;
every function takes `conv`, a dict of overrides, so a planted error is this module with one
entry changed and never a second copy of the code.
"""
from collections import namedtuple

import numpy as np

CONVENTIONS = dict(
    swap_rule=True,       # pair features: source and target exchanged when acos|a1| > acos|a2|
    weight_power=2,       # FPFH: an SPFH weighs 1 / d^2
    incr_minus=1,         # SPFH increment 100 / (k - 1)
    skip_self=True,       # SPFH skips the pair (p, p)
    lrf_weighted=True,    # SHOT frame: covariance weights r - d
    flip_x=True,          # SHOT frame: x takes the sign of the majority
    azimuth_side=1,       # SHOT: the azimuth side bin is the next sector
    radial_knot=0.25,     # SHOT: inner radial knot at r / 4 (outer: 1 - that)
    cosine_wrap=10,       # SHOT: cosine side bins wrap modulo 10
)

COND_FLOOR = 1e-2         # FPFH: a pair conditioned worse than this is ambiguous for its block


def _conv(conv):
    c = dict(CONVENTIONS)
    if conv:
        unknown = set(conv) - set(c)
        if unknown:
            raise KeyError(sorted(unknown))
        c.update(conv)
    return c


def _f64(a):
    return np.asarray(a, np.float64)


def pairwise_d2(A, B):
    """(len(A), len(B)) squared distances from coordinate differences (no |a|^2 + |b|^2 - 2ab)."""
    A, B = _f64(A), _f64(B)
    out = np.empty((len(A), len(B)))
    step = max(1, 2_000_000 // max(1, len(B)))
    with np.errstate(invalid="ignore"):
        for i in range(0, len(A), step):
            d = A[i:i + step, None, :] - B[None, :, :]
            out[i:i + step] = (d * d).sum(2)
    return out


def radius_margin(P, Q, r):
    """Smallest |d^2 - r^2| / r^2 over every (query, point) pair with finite coordinates."""
    d2 = pairwise_d2(Q, P)
    rr = float(r) * float(r)
    d2 = d2[np.isfinite(d2)]
    return float(np.min(np.abs(d2 - rr)) / rr) if d2.size else np.inf


# ---- A.1 radius search --------------------------------------------------------------------

def neighbours(P, q, r):
    """Brute force d^2 < r^2: (indices ascending by (d^2, index), distances, margin) with margin the
    smallest relative distance of any d^2 to r^2.  A non-finite query has no neighbours."""
    P, q = _f64(P), _f64(q)
    if not np.isfinite(q).all():
        return np.empty(0, np.int64), np.empty(0), np.inf
    d = P - q
    with np.errstate(invalid="ignore"):
        d2 = (d * d).sum(1)
        rr = float(r) * float(r)
        idx = np.flatnonzero(d2 < rr)
    idx = idx[np.lexsort((idx, d2[idx]))]
    fin = d2[np.isfinite(d2)]
    margin = float(np.min(np.abs(fin - rr)) / rr) if fin.size else np.inf
    return idx, np.sqrt(d2[idx]), margin


# ---- A.2 normals --------------------------------------------------------------------------

Normals = namedtuple("Normals", "n curvature gap trace pmax2 k facing")


def normals(P, r, viewpoint=(0.0, 0.0, 0.0)):
    """Normal and curvature of every point: two-pass covariance of the neighbourhood, eigh, the
    eigenvector of the smallest eigenvalue turned towards the viewpoint, curvature |l0 / trace|;
    NaN for fewer than 3 neighbours.  Per row also: the eigen-gap l1 - l0, the trace, max |p|^2
    over the neighbourhood, the neighbour count and |n . (vp - p)| / |vp - p|."""
    P = _f64(P)
    vp = _f64(viewpoint)
    n = len(P)
    cov = np.zeros((n, 3, 3))
    pmax2 = np.full(n, np.nan)
    k = np.zeros(n, np.int64)
    for i in range(n):
        idx, _, _ = neighbours(P, P[i], r)
        k[i] = len(idx)
        if len(idx) < 3:
            continue
        nb = P[idx]
        x = nb - nb.mean(0)
        cov[i] = x.T @ x / len(idx)
        pmax2[i] = (nb * nb).sum(1).max()
    lam, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0].copy()
    to_vp = vp - P
    s = (nrm * to_vp).sum(1)
    nrm[s < 0] *= -1.0
    trace = lam.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(trace != 0, np.abs(lam[:, 0] / trace), 0.0)
        facing = np.abs(s) / np.linalg.norm(to_vp, axis=1)
    gap = lam[:, 1] - lam[:, 0]
    bad = k < 3
    nrm[bad] = np.nan
    for a in (curv, gap, trace, facing):
        a[bad] = np.nan
    return Normals(nrm, curv, gap, trace, pmax2, k, facing)


# ---- A.3 FPFH -----------------------------------------------------------------------------

def _dot(a, b):
    return (a * b).sum(-1)


def pair_features(p1, n1, p2, n2, conv=None):
    """Darboux-frame features of the pairs (rows): f1 = theta = atan2(w . nt, u . nt),
    f2 = alpha = v . nt, f3 = phi = u . dp / |dp|, with u the source normal, v = dp x u / |dp x u|,
    w = u x v, and source and target exchanged (dp negated) when acos|a1| > acos|a2|.  A pair
    with |dp| = 0 or |dp x u| = 0 fails and returns f1 = f2 = f3 = 0.

    Returns (f1, f2, f3, ok, (swap_margin, v_sine, theta_radius)): | |a1| - |a2| |, the distance
    to the swap decision; |dp x u| / |dp|, what v is divided by; hypot(w . nt, u . nt), the
    radius atan2 works at.  They are inf for a failed pair (its zeros are exact)."""
    c = _conv(conv)
    p1, n1, p2, n2 = (np.atleast_2d(_f64(a)) for a in (p1, n1, p2, n2))
    dp = p2 - p1
    f4 = np.linalg.norm(dp, axis=1)
    ok = f4 > 0
    f4s = np.where(ok, f4, 1.0)
    a1 = _dot(n1, dp) / f4s
    a2 = _dot(n2, dp) / f4s
    with np.errstate(invalid="ignore"):
        swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))   # NaN (|a| > 1) compares false
    if not c["swap_rule"]:
        swap = np.zeros_like(swap)
    sw = swap[:, None]
    u = np.where(sw, n2, n1)
    nt = np.where(sw, n1, n2)
    dps = np.where(sw, -dp, dp)
    f3 = np.where(swap, -a2, a1)
    v = np.cross(dps, u)
    vn = np.linalg.norm(v, axis=1)
    ok = ok & (vn > 0)
    v = v / np.where(vn > 0, vn, 1.0)[:, None]
    w = np.cross(u, v)
    f2 = _dot(v, nt)
    y, x = _dot(w, nt), _dot(u, nt)
    f1 = np.arctan2(y, x)
    f1, f2, f3 = (np.where(ok, f, 0.0) for f in (f1, f2, f3))
    inf = np.inf
    cond = (np.where(ok, np.abs(np.abs(a1) - np.abs(a2)), inf), np.where(ok, vn / f4s, inf),
            np.where(ok, np.hypot(y, x), inf))
    return f1, f2, f3, ok, cond


def fpfh_interval(P, N, Q, r, same_as_surface=False, tau=1e-4, conv=None):
    """FPFH-33 of the queries Q over the surface (P, N) as an interval: (lo, hi, ambiguous_share),
    lo and hi (nq, 33) on the 0-100 scale with lo <= FPFH <= hi for every evaluation whose pair
    features are within tau bin units of the exact ones, ambiguous_share = max(hi - lo) per row.

    SPFH(p) over the neighbours q != p of p adds 100 / (k - 1) per pair to one bin of each of the
    three 11-bin blocks; FPFH(q) = sum over the neighbours of q with d^2 != 0 of SPFH / d^2, each
    block scaled to 100.  A pair whose bin coordinate is farther than tau from every bin edge adds
    to lo and hi of its bin; one nearer to an edge adds to hi of both adjacent bins only.  A pair
    whose swap decision is within tau (| |a1| - |a2| | <= tau), or one of whose other conditioning
    numbers is below COND_FLOOR, adds to hi of all 11 bins of each block it touches and to no lo.
    The mass of a block does not depend on the bins, so the scaling is exact.  same_as_surface:
    the queries are the surface points (Q is not read).  A query without neighbours gives a NaN row.

    A failed pair (pair_features) is binned with its zeros, in the middle bin of each block, and
    counts in the mass.  SURVEY A.3 says such a pair is skipped; PCL 1.7's FPFHEstimation calls
    computePairFeatures through a wrapper that drops its return value, which is the reading DESIGN.md
    section 5 records and the restatement follows.  On this one point the statement takes the
    restatement's reading instead of testing it, and no case of tests/f64_cases.py holds a failed
    pair (no duplicate points, no normal along a pair's direction): it is not pinned here."""
    c = _conv(conv)
    P, N = _f64(P), _f64(N)
    Q = P if same_as_surface else _f64(Q)
    rr = float(r) * float(r)
    d2q = pairwise_d2(Q, P)
    with np.errstate(invalid="ignore"):
        mq = d2q < rr
    need = np.arange(len(P)) if same_as_surface else np.flatnonzero(mq.any(0))
    ms = pairwise_d2(P[need], P) < rr
    k = ms.sum(1)
    rows, cols = np.nonzero(ms)
    if c["skip_self"]:
        keep = need[rows] != cols
        rows, cols = rows[keep], cols[keep]
    with np.errstate(divide="ignore"):
        incr = (100.0 / (k - c["incr_minus"]))[rows]
    src = need[rows]
    f1, f2, f3, _, (swap_margin, v_sine, theta_radius) = pair_features(P[src], N[src], P[cols], N[cols], conv)
    coord = np.stack([11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0], 1)
    nan = np.isnan(coord)                       # a NaN feature lands in bin 0
    coord = np.where(nan, 0.5, coord)
    bins = np.clip(np.floor(coord), 0, 10).astype(np.int64)
    edge = np.rint(coord)
    near = (np.abs(coord - edge) <= tau) & (edge >= 1) & (edge <= 10) & ~nan
    edge = edge.astype(np.int64)
    whole = np.zeros(coord.shape, bool)
    whole[:, :] |= (swap_margin <= tau)[:, None]      # every feature depends on the swap
    whole[:, :2] |= (v_sine < COND_FLOOR)[:, None]    # f1 and f2 are read off v
    whole[:, 0] |= theta_radius < COND_FLOOR          # f1 is an angle at this radius
    ns = len(need)
    lo_s = np.zeros((ns, 33))
    hi_s = np.zeros((ns, 33))
    mass = np.zeros((ns, 3))
    for b in range(3):
        mass[:, b] = np.bincount(rows, incr, ns)
        sure = ~whole[:, b] & ~near[:, b]
        np.add.at(lo_s, (rows[sure], 11 * b + bins[sure, b]), incr[sure])
        np.add.at(hi_s, (rows[sure], 11 * b + bins[sure, b]), incr[sure])
        ne = near[:, b] & ~whole[:, b]
        np.add.at(hi_s, (rows[ne], 11 * b + edge[ne, b] - 1), incr[ne])
        np.add.at(hi_s, (rows[ne], 11 * b + edge[ne, b]), incr[ne])
        wh = whole[:, b]
        hi_s[:, 11 * b:11 * b + 11] += np.bincount(rows[wh], incr[wh], ns)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        wq = np.where(mq & (d2q > 0), d2q ** (-0.5 * c["weight_power"]), 0.0)[:, need]
    lo, hi, m = wq @ lo_s, wq @ hi_s, wq @ mass
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.repeat(np.where(m > 0, 100.0 / m, 1.0), 11, axis=1)
    lo, hi = lo * scale, hi * scale
    empty = ~mq.any(1)
    lo[empty] = np.nan
    hi[empty] = np.nan
    return lo, hi, (hi - lo).max(1)


# ---- A.7 SHOT -----------------------------------------------------------------------------

def shot_lrf(P, c, r, conv=None):
    """SHOT local reference frame of the point c over the surface P: the (r - d)-weighted
    covariance of the neighbours not equal to c, eigh, x the eigenvector of the largest and z of
    the smallest eigenvalue, each turned to the side most neighbours lie on (a tie: the five
    neighbours around the median distance decide), y = z x x.  NaN for fewer than 5 such points.

    Returns (rf (9,) = x, y, z, (gap, x_margin, z_margin)): min(l1 - l0, l2 - l1) / l2 and
    |2 count - n| of either sign vote."""
    cv = _conv(conv)
    P, c = _f64(P), _f64(c)
    idx, d, _ = neighbours(P, c, r)
    v = P[idx] - c
    keep = (v != 0).any(1)
    v, d = v[keep], d[keep]
    n = len(v)
    if n < 5:
        return np.full(9, np.nan), (np.nan, np.nan, np.nan)
    w = float(r) - d if cv["lrf_weighted"] else np.ones(n)
    lam, vec = np.linalg.eigh((v * w[:, None]).T @ v / w.sum())

    def vote(axis):
        s = v @ axis
        margin = 2 * int((s >= 0).sum()) - n
        if margin == 0:
            mid = n // 2
            margin = 1 if int((s[mid - 2:mid + 3] > 0).sum()) >= 3 else -1
            return margin < 0, 0
        return margin < 0, abs(margin)

    x, z = vec[:, 2], vec[:, 0]
    flip, xm = vote(x)
    if flip and cv["flip_x"]:
        x = -x
    flip, zm = vote(z)
    if flip:
        z = -z
    rf = np.concatenate([x, np.cross(z, x), z])
    return rf, (float(min(lam[1] - lam[0], lam[2] - lam[1]) / lam[2]), xm, zm)


def _interp(u, main, size, periodic, side_step=1):
    """One axis of the multilinear vote: bin centres at 0 .. size - 1, coordinate u, main bin
    `main`.  Returns (weight of the main bin, side bin or -1, weight of the side bin)."""
    delta = u - main
    side = main + side_step * np.where(delta > 0, 1, -1)
    side = side % size if periodic else np.where((side >= 0) & (side < size), side, -1)
    return 1.0 - np.abs(delta), side, np.abs(delta)


def shot352(P, N, c, rf, r, conv=None):
    """SHOT-352 of the point c in the frame rf (9,): an 8 azimuth x 2 radial x 2 elevation x 11
    cosine tensor, L2-normalised, flattened as ((az * 4 + radial * 2 + elev) * 11 + cos).

    Every neighbour with a finite normal and d > 0 votes with linear interpolation along four
    axes -- the cosine of its normal to z (bin centres 0 .. 10 of (1 + cos) * 5, side bins modulo
    10), the radius (centres at r/4 and 3r/4), the elevation (centres at 45 and 135 degrees, the
    upper hemisphere is bin 1) and the azimuth (sector centres at -7 pi/8 + sel pi/4, offset
    clamped to +-0.5, periodic): the main bin gets the sum of the four main weights, and along each
    axis the adjacent bin, where there is one, the complement.  NaN for fewer than 5 neighbours."""
    cv = _conv(conv)
    P, N, c, rf = _f64(P), _f64(N), _f64(c), _f64(rf)
    idx, d, _ = neighbours(P, c, r)
    if len(idx) < 5 or not np.isfinite(rf).all():
        return np.full(352, np.nan)
    nrm = N[idx]
    use = np.isfinite(nrm).all(1) & (d > 0)
    idx, d, nrm = idx[use], d[use], nrm[use]
    x, y, z = rf[0:3], rf[3:6], rf[6:9]
    delta = P[idx] - c
    xl, yl, zl = delta @ x, delta @ y, delta @ z
    r = float(r)

    cosb = (1.0 + np.clip(nrm @ z, -1.0, 1.0)) * 10.0 / 2.0
    i_cos = np.floor(cosb + 0.5).astype(np.int64)
    w_cos, s_cos, sw_cos = _interp(cosb, i_cos, cv["cosine_wrap"], True)

    knot = cv["radial_knot"] * r
    u_rad = (d - knot) / (r - 2.0 * knot)
    i_rad = (d > r / 2.0).astype(np.int64)
    w_rad, s_rad, sw_rad = _interp(u_rad, i_rad, 2, False)

    incl = np.arccos(np.clip(zl / d, -1.0, 1.0))
    i_el = (zl > 0).astype(np.int64)
    u_el = 1.0 - (incl - np.pi / 4.0) / (np.pi / 2.0)      # 1 at 45 degrees, 0 at 135
    w_el, s_el, sw_el = _interp(u_el, i_el, 2, False)

    az = np.arctan2(yl, xl)
    planar = (xl != 0) | (yl != 0)
    i_az = np.clip(np.floor((az + np.pi) / (np.pi / 4.0)), 0, 7).astype(np.int64)
    u_az = (az + 7.0 * np.pi / 8.0) / (np.pi / 4.0)
    u_az = i_az + np.clip(u_az - i_az, -0.5, 0.5)
    w_az, s_az, sw_az = _interp(u_az, i_az, 8, True, cv["azimuth_side"])
    w_az, sw_az = np.where(planar, w_az, 0.0), np.where(planar, sw_az, 0.0)

    h = np.zeros((8, 2, 2, 11))
    np.add.at(h, (i_az, i_rad, i_el, i_cos), w_cos + w_rad + w_el + w_az)
    np.add.at(h, (i_az, i_rad, i_el, s_cos), sw_cos)
    m = s_rad >= 0
    np.add.at(h, (i_az[m], s_rad[m], i_el[m], i_cos[m]), sw_rad[m])
    m = s_el >= 0
    np.add.at(h, (i_az[m], i_rad[m], s_el[m], i_cos[m]), sw_el[m])
    np.add.at(h, (s_az[planar], i_rad[planar], i_el[planar], i_cos[planar]), sw_az[planar])
    h = h.reshape(352)
    return h / np.sqrt((h * h).sum())
