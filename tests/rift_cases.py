"""Small synthetic inputs of the intensity-gradient and RIFT tests (plain numpy, no GPU), for the
search radius R.  Surfaces are (x, y, z) float32 tuples, gradients and normals likewise."""
import numpy as np

import pfh_cases as C
from spin_cases import Q0, R, STEP, f32, offset, points  # noqa: F401  (offsets by powers of two: exact)

NAN_BITS = 0x7fc00000  # how the kernels and the restatement write a NaN


def vectors(n, v):
    """n copies of the vector v."""
    a = np.repeat(np.asarray(v, np.float32)[None], n, axis=0)
    return f32(a[:, 0], a[:, 1], a[:, 2])


def random_vectors(n, seed, scale=1.0):
    v = np.random.default_rng(seed).normal(size=(n, 3)) * scale
    return f32(v[:, 0], v[:, 1], v[:, 2])


def intensities(n, seed):
    """Intensities as PointXYZRGBtoXYZI gives them: 0 .. 255."""
    return np.random.default_rng(seed).uniform(0.0, 255.0, n).astype(np.float32)


def pair(gradient, step=(STEP, 0.0, 0.0), centre_gradient=(0.0, 0.0, 0.0)):
    """The centre Q0 (row 0, a zero gradient unless given: it adds zeros) and one neighbour at Q0 + step
    with `gradient`.  With step = (STEP, 0, 0): d = D * 2^-6 / (R + eps), 1.25 for D = 4."""
    xyz = points(Q0, offset(*step))
    g = np.asarray([centre_gradient, gradient], np.float32)
    return xyz, f32(g[:, 0], g[:, 1], g[:, 2])


def plane_case(a=2.0, b=-0.5, side=8, spacing=2.0 ** -8):
    """side x side points on z = 3 around Q0 with I = a x + b y: every coordinate, sum, centroid
    (side * side is a power of two) and intensity is exact in float32, every point sees every other
    (the diagonal 7 sqrt(2) / 256 = 0.039 < R), the normals are +z.  The system has rank two (every
    p_z is exactly 0), A = diag(s, s, 0): the gradient is (a, b, 0)."""
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    x = Q0[0] + i.ravel() * spacing
    y = Q0[1] + j.ravel() * spacing
    z = np.full(side * side, Q0[2])
    xyz = f32(x, y, z)
    inten = (np.float32(a) * xyz[0] + np.float32(b) * xyz[1]).astype(np.float32)
    assert np.array_equal(inten.astype(np.float64), a * x + b * y)
    return dict(xyz=xyz, intensity=inten, normals=vectors(side * side, (0.0, 0.0, 1.0)), want=(a, b, 0.0))


def order_case(k=320, blobs=8):
    """`blobs` blobs of k points, each in a cube whose diagonal is below R, one query per blob (its
    first point), with random intensities, gradients and unit normals: a few hundred additions per
    accumulator, so the neighbour order decides low bits."""
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), 400 + 2 * s) for s in range(blobs)]
    xyz, _, rows = C.concat(parts)
    n = len(xyz[0])
    qr = np.array([lo for lo, _ in rows])
    return dict(xyz=xyz, rows=qr, q=tuple(v[qr] for v in xyz), intensity=intensities(n, 398),
                gradients=random_vectors(n, 399, 30.0), normals=C.unit_normals(n, 397),
                qnormals=C.unit_normals(blobs, 396), k=k)


def blobs_case(ks, seed):
    """One blob of each size in ks, 1 m apart: a point of a blob of k points has exactly k neighbours."""
    parts = [C.blob(k, (1.0 + s, 2.0, 3.0), seed + 2 * s) for s, k in enumerate(ks)]
    xyz, _, rows = C.concat(parts)
    n = len(xyz[0])
    return dict(xyz=xyz, rows=rows, intensity=intensities(n, seed - 1), gradients=random_vectors(n, seed - 2, 30.0),
                normals=C.unit_normals(n, seed - 3))
