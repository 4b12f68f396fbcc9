"""Small synthetic inputs of the shape-context tests (plain numpy, no GPU) and a direct float64
statement of the bin a lone neighbour falls into.  Surfaces are (x, y, z) float32 tuples, normals
likewise; R, RMIN and RHO are the reference's radii."""
import numpy as np

import pfh_cases as C
from spin_cases import Q0, STEP, f32, offset, points  # noqa: F401  (offsets by powers of two: exact)

R = 0.08
RMIN = R / 10
RHO = R / 5
NAN_BITS = 0x7fc00000  # how the kernels and the restatement write a NaN
EPS = np.float32(2.0 ** -23)
LEN = 1980


def vectors(n, v):
    a = np.repeat(np.asarray(v, np.float32)[None], n, axis=0)
    return f32(a[:, 0], a[:, 1], a[:, 2])


def tables64(r=R, rmin=RMIN):
    """The tables in float64, stated directly: radii (16), theta_div (12), phi_div (13), lut (11, 15)."""
    j = np.arange(16)
    radii = np.exp(np.log(rmin) + (j / 15.0) * np.log(r / rmin))
    theta_div = np.arange(12) * (180.0 / 11.0)
    phi_div = np.arange(13) * 30.0
    d_phi = np.deg2rad(30.0)
    d_theta = np.cos(np.deg2rad(theta_div[:-1])) - np.cos(np.deg2rad(theta_div[1:]))
    d_r = radii[1:] ** 3 - radii[:-1] ** 3
    lut = 1.0 / np.cbrt(d_phi * d_theta[:, None] * d_r[None, :])
    return radii, theta_div, phi_div, lut


def first_division(v, div):
    """The contract's search: the first i >= 1 with v <= div[i], minus 1; 0 when none (a NaN too)."""
    for i in range(1, len(div)):
        if v <= div[i]:
            return i - 1
    return 0


def bin_of(p, o, x, n, t):
    """(l, k, j) of the neighbour p of the query o in the frame (x, n), in float64 on the float32
    tables t: for neighbours away from every bin edge."""
    p, o, x, n = (np.asarray(v, np.float64) for v in (p, o, x, n))
    po = p - o
    r = np.linalg.norm(po)
    proj = po - n.dot(po) * n
    proj /= np.linalg.norm(proj)
    c = np.cross(x, proj)
    phi = np.degrees(np.arctan2(np.linalg.norm(c), x.dot(proj)))
    if c.dot(n) < 0:
        phi = 360.0 - phi
    theta = np.degrees(np.arccos(np.clip(n.dot(po / r), -1.0, 1.0)))
    return first_division(phi, t.phi_div), first_division(theta, t.theta_div), first_division(r, t.radii)


def flat(l, k, j):
    return l * 165 + k * 15 + j


def lone_neighbour(step=(STEP, STEP, STEP), normal=(0.0, 0.0, 1.0)):
    """The query Q0 is row 0 of the surface (d2 = 0: skipped, but the nearest, so its normal makes the
    frame) and one neighbour at Q0 + step.  Returns the surface and its normals."""
    return points(Q0, offset(*step)), vectors(2, normal)


def order_case(k=1100, blobs=3, seed=700):
    """`blobs` dense blobs of k points in a cube of side 0.04 (every point within R = 0.08 of every
    other), one query per blob: about k / 50 additions per occupied bin on average and many more in
    the outer shells, so the neighbour order decides low bits."""
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), seed + 2 * s, side=0.04) for s in range(blobs)]
    xyz, nrm, rows = C.concat(parts)
    qr = np.array([lo for lo, _ in rows])
    return dict(xyz=xyz, normals=nrm, q=tuple(v[qr] for v in xyz), k=k)


def rim_case(seed=710):
    """One query at Q0.  Inside its ball: Q0 itself and a neighbour at distance 0.075 (near the rim,
    R = 0.08).  Outside the ball, but within RHO = 0.016 of that neighbour: five more points at
    distance 0.085 .. 0.089 from the query.  The neighbour's density is 6; a count over the query's
    ball alone would give 1.  Also one point with a NaN coordinate beside the neighbour: counted
    nowhere."""
    rng = np.random.default_rng(seed)
    near = offset(0.075)
    outside = [offset(0.085 + 0.001 * i, rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004)) for i in range(5)]
    xyz = points(Q0, near, *outside, (np.nan, near[1], near[2]))
    return dict(xyz=xyz, normals=vectors(len(xyz[0]), (0.0, 0.0, 1.0)), q=points(Q0), density=6)
