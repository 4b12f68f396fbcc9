"""The clouds shared by the boundary-point tests (tests/test_boundary_ref.py, test_abi_boundary.py,
test_gpu_boundary.py): small closed forms whose flags follow from the geometry, placed through the
contract's own plane axes so that a neighbour's angle is the one the case names."""
import math

import numpy as np

F = np.float32
PI_F = F(math.pi)
R = 0.05          # the radius of the ring cases
RHO = 0.02        # ... and the rings' own


def f32(*a):
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in a)


def points(*p):
    """Points as three float32 columns."""
    a = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    return f32(a[:, 0], a[:, 1], a[:, 2])


def plane_axes(n):
    """The contract's (u, v) of a normal, in float32 as it states them."""
    n = np.asarray(n, dtype=np.float32)
    m, am = 0, abs(n[0])
    for i in (1, 2):
        if abs(n[i]) > am:
            m, am = i, abs(n[i])
    s = 1 if m == 0 else 0
    inv = F(1.0) / np.sqrt(F(n[s] * n[s]) + F(n[m] * n[m]))
    v = np.zeros(3, np.float32)
    v[m] = -n[s] * inv
    v[s] = n[m] * inv
    u = np.array([F(n[1] * v[2]) - F(n[2] * v[1]), F(n[2] * v[0]) - F(n[0] * v[2]), F(n[0] * v[1]) - F(n[1] * v[0])], F)
    return u, v


def lattice():
    """9 x 9 planar lattice, spacing 0.01, normals +z; at r = 0.025 the 32 rim points are boundary
    points at pi / 2 (a rim point's neighbours fill a half plane at most) and the 49 interior points
    (neighbours every 45 degrees or closer) are not.  Returns xyz, normals, the rim mask."""
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    i, j = i.ravel(), j.ravel()
    xyz = f32(0.01 * i, 0.01 * j, np.zeros(81))
    nrm = f32(np.zeros(81), np.zeros(81), np.ones(81))
    rim = (i == 0) | (i == 8) | (j == 0) | (j == 8)
    return xyz, nrm, rim


def ring(angles, n=(0.0, 0.0, 1.0), centre=(0.0, 0.0, 0.0), rho=RHO, duplicates=0, with_centre=True):
    """A centre and one neighbour at every angle (radians, as atan2f(v . d, u . d) will see it to a few
    1e-7) on the circle of radius rho in the plane of the contract's axes of n.  duplicates: further
    copies of the centre.  Returns the surface xyz, the query (the centre) and its normal."""
    u, v = plane_axes(n)
    c = np.asarray(centre, dtype=np.float64)
    a = np.asarray(angles, dtype=np.float64).reshape(-1, 1)
    p = c + rho * (np.cos(a) * u.astype(np.float64) + np.sin(a) * v.astype(np.float64))
    own = np.repeat(c.reshape(1, 3), duplicates + (1 if with_centre else 0), axis=0)
    s = np.concatenate([own, p]) if len(a) else own
    return points(*s), points(c), points(n)


def even(m, phase=0.1):
    """m equally spaced angles in (-pi, pi)."""
    return -math.pi + phase + 2 * math.pi * np.arange(m) / m


# normals whose largest component is x, y and z in turn, and ties of |n_i| (the first largest wins)
NORMALS = {
    "x": (0.8, 0.36, -0.48), "y": (0.36, -0.8, 0.48), "z": (-0.48, 0.36, 0.8),
    "tie_xy": (0.6, 0.6, 0.52915026), "tie_yz": (0.2, -0.69282, 0.69282), "tie_all": (0.57735, 0.57735, 0.57735),
    "minus_z": (0.0, 0.0, -1.0),
}


def holed_plane(n=4096, seed=20, hole=0.2, sigma=0.002):
    """n points uniform in the unit square minus a disc of radius `hole` about its middle, z noise
    sigma: boundary points along the square's edges and the hole's rim (r = 0.05)."""
    rng = np.random.default_rng(seed)
    xy = np.empty((0, 2))
    while len(xy) < n:
        c = rng.random((2 * n, 2))
        xy = np.concatenate([xy, c[np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5) >= hole]])
    xy = xy[:n]
    return f32(xy[:, 0], xy[:, 1], rng.normal(0.0, sigma, n))


def bin_edge_angles():
    """Neighbours whose angles are -pi_f, +pi_f, -0 and +0 to the bit under the normal +z (u = +y,
    v = +x: the angle is atan2f(dx, dy)), about a query at the origin, r = 10: dx = +0 below the query
    (+pi_f), dx = -1e-30 below it (the quotient vanishes beside pi: -pi_f), dx = +0 above it (+0), and
    dx = the smallest negative denormal above it, whose quotient by 4 rounds to zero (-0)."""
    tiny = np.float32(-1.0e-30)
    denorm = -np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]
    pts = {"+pi": (0.0, -4.0, 0.0), "-pi": (tiny, -4.0, 0.0), "+0": (0.0, 4.0, 0.0), "-0": (denorm, 4.0, 0.0)}
    return pts, 10.0
