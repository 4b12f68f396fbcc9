"""Small synthetic inputs of the moment-invariant and principal-curvature tests (plain numpy, no
GPU), for the search radius R.  Surfaces and normals are (x, y, z) float32 tuples."""
import numpy as np

import pfh_cases as C
from rift_cases import vectors  # noqa: F401
from spin_cases import Q0, R, STEP, f32, offset, points  # noqa: F401  (offsets by powers of two: exact)

NAN_BITS = 0x7fc00000  # how the kernels and the restatement write a NaN
Z = (0.0, 0.0, 1.0)


def axis_case(a=2.0 ** -6, b=2.0 ** -7, c=2.0 ** -5):
    """Q0 +- a e_x, +- b e_y, +- c e_z and the centre Q0: k = 7.  The coordinate sums 7, 14 and 21
    are exact; times fl(1 / 7) they round to 1, 2 and 3 + d with d = 2^-22.  So t0 and t1 are
    exact, t2 = +-c - d: (c - d)^2 and (c + d)^2 round to c^2 (1 -+ 2^-16 (2^-5 / c)) for the
    powers of two used here and add up to 2 c^2, the other d^2 terms vanish below the sums' last
    bit and the mixed products with d cancel in pairs:
    mu200 = 2 a^2, mu020 = 2 b^2, mu002 = 2 c^2, the mixed sums 0 in either walking direction
    (tests/test_moments_ref.py checks it).  Returns the surface and (j1, j2, j3)."""
    xyz = points(Q0, offset(a), offset(-a), offset(0, b), offset(0, -b), offset(0, 0, c), offset(0, 0, -c))
    a2, b2, c2 = a * a, b * b, c * c
    return xyz, (2 * (a2 + b2 + c2), 4 * (a2 * b2 + a2 * c2 + b2 * c2), 8 * a2 * b2 * c2)


def diagonal_case(a=STEP):
    """Q0 +- (a, a, 0) (k = 2, the query Q0 is no surface point): mu200 = mu020 = mu110 = 2 a^2, so
    j1 = 4 a^2 and j2 = j3 = 0 exactly."""
    return points(offset(a, a), offset(-a, -a)), (4 * a * a, 0.0, 0.0)


def ring(k=8, step=2.0 ** -8):
    """k distinct points Q0 + i step e_x (row 0 is Q0), all within R of Q0."""
    return points(*[offset(i * step) for i in range(k)])


def spread_case(m):
    """Eight neighbours of Q0 with query normal +z: m pairs of normals (+-0.5, 0, 1), the rest
    (0, 0, 1).  The projections are (+-0.5, 0, 0) and 0, their centroid 0, the covariance
    diag(2 m 0.25, 0, 0): direction (1, 0, 0), pc1 = 2 m 0.25 / 8, pc2 = 0, exactly.
    Returns the surface, its normals and the row."""
    assert 1 <= m <= 4
    n = np.zeros((8, 3), np.float32)
    n[:, 2] = 1.0
    n[:m, 0], n[m:2 * m, 0] = 0.5, -0.5
    # (the pairs are spread over the FLANN order, not adjacent in it)
    n = n[np.random.default_rng(11).permutation(8)]
    return ring(8), f32(n[:, 0], n[:, 1], n[:, 2]), (1.0, 0.0, 0.0, 2 * m * 0.25 / 8, 0.0)


def order_case(k=320, blobs=8):
    """`blobs` blobs of k points, each in a cube whose diagonal is below R, one query per blob (its
    first point), with random unit normals: a few hundred additions per accumulator, so the
    neighbour order decides low bits."""
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), 600 + 2 * s) for s in range(blobs)]
    xyz, nrm, rows = C.concat(parts)
    qr = np.array([lo for lo, _ in rows])
    return dict(xyz=xyz, normals=nrm, rows=qr, q=tuple(v[qr] for v in xyz), qnormals=C.unit_normals(blobs, 596), k=k)


def blobs_case(ks, seed):
    """One blob of each size in ks, 1 m apart: a point of a blob of k points has exactly k neighbours."""
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), seed + 2 * s) for s, k in enumerate(ks)]
    xyz, nrm, rows = C.concat(parts)
    return dict(xyz=xyz, normals=nrm, rows=rows)


def smooth_blobs(blobs=16, k=40, seed=620):
    """Blobs whose normals scatter a little around +z, every point a query with its own normal: the
    covariances of a smooth surface, on which (root2 * scale) / scale often differs from root2."""
    rng = np.random.default_rng(seed)
    parts = []
    for s in range(blobs):
        xyz, _ = C.blob(k, (1.0 + s, 2.0, 3.0), seed + 1 + s)
        v = np.asarray(Z) + rng.normal(scale=0.15, size=(k, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        parts.append((xyz, f32(v[:, 0], v[:, 1], v[:, 2])))
    xyz, nrm, _ = C.concat(parts)
    return dict(xyz=xyz, normals=nrm)
