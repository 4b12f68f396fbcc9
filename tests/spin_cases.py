"""Small synthetic inputs of the spin-image tests (plain numpy, no GPU), for the search radius R.
Surfaces are (x, y, z) float32 tuples, axes (ax, ay, az) float32 tuples."""
import math

import numpy as np

import pfh_cases as C

R = 0.05
Q0 = (1.0, 2.0, 3.0)   # a query whose offsets by powers of two are exact in float32
STEP = 2.0 ** -6       # 0.015625 < R / sqrt(2): its square and its norm are exact
Z = (0.0, 0.0, 1.0)


def f32(*a):
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in a)


def bin_size(r=R, w=8):
    """`search_radius_ / image_width_ / sqrt (2.0)`, left to right in double."""
    return r / w / math.sqrt(2.0)


def points(*pts):
    """Points (x, y, z) -> a surface."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    return f32(p[:, 0], p[:, 1], p[:, 2])


def offset(dx=0.0, dy=0.0, dz=0.0, q=Q0):
    return (q[0] + dx, q[1] + dy, q[2] + dz)


def axes(n, axis=Z):
    a = np.repeat(np.asarray(axis, np.float32)[None], n, axis=0)
    return f32(a[:, 0], a[:, 1], a[:, 2])


def order_case(k=320, blobs=8):
    """GPU case 4 (and the CPU test that proves its teeth): `blobs` blobs of k points, each in a cube
    whose diagonal is below R, one query per blob (its first point) with a generic unit axis."""
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), 300 + 2 * s) for s in range(blobs)]
    xyz, _, rows = C.concat(parts)
    qr = np.array([lo for lo, _ in rows])
    return dict(xyz=xyz, q=tuple(v[qr] for v in xyz), axes=C.unit_normals(blobs, 299), k=k)


def cos_one_row(xyz, q, r=R, w=8):
    """The row of query q when every cosine is exactly 1.0 (the NaN-axis rule), stated directly:
    alpha = 0, beta = direction_norm, so the mass of a neighbour is (1 - b, b) in alpha_bin 0.
    Returns (raw (S,) float64 in output order, k)."""
    x, y, z = (np.asarray(v, np.float32) for v in xyz)
    qx, qy, qz = (np.float32(v) for v in q)
    dx, dy, dz = qx - x, qy - y, qz - z
    d2 = ((np.float32(0.0) + dx * dx) + dy * dy) + dz * dz            # FLANN's L2_Simple
    nb = np.flatnonzero(d2 < np.float32(r * r))
    nb = nb[np.lexsort((nb, d2[nb]))]                                   # (d2, index) ascending
    bs, cols = bin_size(r, w), 2 * w + 1
    m = np.zeros(((w + 1), cols), np.float64)
    for i in nb:
        ex, ey, ez = x[i] - qx, y[i] - qy, z[i] - qz
        dn = float(np.sqrt((ex * ex + ez * ez) + (ey * ey + np.float32(0.0))))  # float32 throughout
        if dn < 10 * float(np.finfo(np.float32).eps):
            continue
        beta = dn * 1.0
        if abs(beta) >= bs * w:
            continue
        bb = int(math.floor(beta / bs)) + w
        assert bb < 2 * w
        b = beta / bs - (bb - w)
        m[0, bb] += (1.0 - 0.0) * (1.0 - b)
        m[0, bb + 1] += (1.0 - 0.0) * b
    return m.ravel(), len(nb)


def support_case():
    """Query Q0 with axis +z, support_angle_cos = 0.5.  Neighbour normals (0, 0, nz) make the cosine
    nz exactly.  Returns xyz, normals, kept: per surface point whether the support test keeps it."""
    rng = np.random.default_rng(77)
    n = 40
    p = np.asarray(Q0) + rng.uniform(-0.0125, 0.0125, (n, 3))
    p[0] = Q0
    nz = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    half = np.float32(0.5)
    nz[1], nz[2] = np.nextafter(half, np.float32(0)), half                  # just below: dropped; at: kept
    nz[3], nz[4] = -np.nextafter(half, np.float32(0)), -half               # counter-directed, the same
    nz[5], nz[6], nz[7] = -1.0, 1.0, np.nan                                 # NaN: the cosine becomes 1.0
    kept = ~(np.abs(nz) < half)                                            # (NaN compares false: kept)
    assert kept[[2, 4, 5, 6, 7]].all() and not kept[[1, 3]].any() and (~kept).sum() > 5
    nx = np.where(np.isnan(nz), np.nan, 0.0)
    return points(*p), f32(nx, nx, nz), kept
