"""Small synthetic inputs of the BOARD tests (plain numpy, no GPU).  Surfaces and normals are
(x, y, z) float32 tuples.

The closed-form cases lie around Q0 = (1, 2, 3) at offsets that are multiples of H = 2^-8, for the
search radius R = 2^-4 = 16 H and the smaller tangent radius TR = 2^-5 = 8 H.  Every coordinate,
every d2, every sum of coordinates and every centroid (the offsets of a case add up to zero, so the
sums are k, 2 k and 3 k) is exact in float32, and every point lies on an axis through Q0, so the
scatter matrix of a case is diagonal and exact: the eigen solve has nothing to iterate, and its
smallest eigenvalue belongs to a coordinate axis.

The margins: (0.85f 0.85f) R^2 = 184.96.. H^2, so of the offsets used only 14 H (196 H^2) lies in
the ring of tangent radius R; (0.85f 0.85f) TR^2 = 46.24.. H^2, so 7 H (49 H^2) lies in the ring of
TR and 5 H (25 H^2) does not.
"""
import numpy as np

import pfh_cases as C
from moments_cases import blobs_case, order_case  # noqa: F401  (blobs of exact k; random unit normals)
from spin_cases import Q0, f32, offset, points  # noqa: F401

H = 2.0 ** -8
R = 2.0 ** -4
TR = 2.0 ** -5
NAN_BITS = 0x7fc00000  # how the kernel and the restatement write a NaN
UP, DOWN = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
TILT = (0.6, 0.0, 0.8)   # z . TILT = 0.8f < 1: the most inclined normal of a case that has it
NAN3 = (np.nan, np.nan, np.nan)

# the rows the cases claim: x axis, y = z cross x, z axis
X_POS = (1, 0, 0, 0, 1, 0, 0, 0, 1)       # x towards +x under z = +z
X_NEG = (-1, 0, 0, 0, -1, 0, 0, 0, 1)     # x towards -x under z = +z
Y_POS = (0, 1, 0, -1, 0, 0, 0, 0, 1)      # x towards +y under z = +z
X_POS_DOWN = (1, 0, 0, 0, -1, 0, 0, 0, -1)  # x towards +x under z = -z

#: the base patch, offsets in H: Q0 itself, then points on the x and the y axis.  The nearest
#: neighbour with d2 > 0 is (2, 0), and it is the only one at its distance
BASE = ((0, 0), (2, 0), (-4, 0), (8, 0), (-6, 0), (0, 4), (0, -4))
#: two nearest neighbours at one distance: (-2, 0) has the lower index
TWINS = ((0, 0), (-2, 0), (2, 0), (6, 0), (-6, 0), (0, 4), (0, -4))
TILTED_ROW = 5  # the row of BASE whose normal the tilted cases replace: (0, 4)


def patch(offsets, normal=UP, special=None):
    """The points Q0 + H (ox, oy, oz) (oz optional) with one normal for all, but for the rows of
    `special` ({row: normal}).  Returns the surface and its normals."""
    pts = [offset(*(H * np.asarray(o + (0,) * (3 - len(o)), np.float64))) for o in offsets]
    n = np.repeat(np.asarray(normal, np.float64)[None], len(pts), axis=0)
    for row, v in (special or {}).items():
        n[row] = v
    return points(*pts), f32(n[:, 0], n[:, 1], n[:, 2])


def closed_form_cases():
    """[(name, surface, normals, tangent_radius, row)] for the query Q0 and the radius R; row is the
    nine floats claimed, a NaN standing for the canonical NaN."""
    nan9 = (np.nan,) * 9
    cases = []

    def add(name, offsets, row, tangent_radius=0.0, **kw):
        xyz, nrm = patch(offsets, **kw)
        cases.append((name, xyz, nrm, tangent_radius, row))

    # equal normals: every cosine is 1, the first neighbour with d2 > 0 gives x
    add("unique nearest neighbour", BASE, X_POS)
    add("two nearest neighbours, the lower index wins", TWINS, X_NEG)
    add("normals -z flip z", BASE, X_POS_DOWN, normal=DOWN)
    add("one tilted normal", BASE, Y_POS, special={TILTED_ROW: TILT})
    # tangent_radius == R: the margin starts at 0.85 R
    ring = BASE + ((14, 0), (-14, 0))
    add("tilted normal inside the margin, neighbours in the ring", ring, X_POS, tangent_radius=R,
        special={TILTED_ROW: TILT})
    add("tilted normal inside the margin, empty ring", BASE, Y_POS, tangent_radius=R, special={TILTED_ROW: TILT})
    # tangent_radius < R: (0, 12) lies between the two radii, (7, 0) alone in the ring of TR
    outer = ((0, 0), (2, 0), (-4, 0), (7, 0), (-5, 0), (0, 4), (0, -4), (0, 12), (0, -12))
    add("tilted normal between the radii is ignored for x", outer, X_POS, tangent_radius=TR, special={7: TILT})
    add("... and decides x with the tangent radius unset", outer, Y_POS, special={7: TILT})
    add("a normal between the radii enters the mean", outer, X_POS_DOWN, tangent_radius=TR,
        special={7: (0.0, 0.0, -16.0)})
    # without (0, +-12) the support is a line along x, whose fit has two zero eigenvalues, the first
    # of them y's: z would be (0, 1, 0)
    add("a position between the radii enters the plane fit", ((0, 0), (2, 0), (-4, 0), (7, 0), (-5, 0), (0, 12), (0, -12)),
        X_POS, tangent_radius=TR)
    six = ((0, 0), (2, 0), (-6, 0), (4, 0), (0, 4), (0, -4))
    add("k = 6", six, X_POS)
    add("k = 5", six[:5], nan9)
    add("all normals NaN", BASE, nan9, normal=NAN3)
    # the NaN normal is the nearest neighbour's; the mean is NaN, so -z normals do not flip z; of the
    # three neighbours at 4 H, (-4, 0) has the lowest index
    add("one NaN normal: no flip, never chosen", BASE, X_NEG, normal=DOWN, special={1: NAN3})
    # (0, 0, 2) with the tilted normal is chosen and lies on the line through Q0 along z; the z extent
    # (8 H^2) is still the smallest of the three
    add("the chosen neighbour lies along z", BASE + ((0, 0, 2), (0, 0, -2)), (np.nan,) * 6 + (0, 0, 1),
        special={7: TILT})
    return cases


def row_bits(row):
    """The claimed row as raw bits, -0 folded into +0 and a NaN written as the canonical one."""
    r = np.asarray(row, np.float32) + np.float32(0.0)
    b = np.ascontiguousarray(r).view(np.uint32).copy()
    b[np.isnan(r)] = NAN_BITS
    return b


def got_bits(rf):
    """A computed row's bits with -0 folded into +0 (the claims do not state the sign of a zero)."""
    r = np.asarray(rf, np.float32)
    b = np.ascontiguousarray(r).view(np.uint32).copy()
    b[r == 0] = 0
    return b


def flann_order(xyz, q, rr):
    """The rows of the surface with d2 < rr around q in (d2, index) order, and their d2 (float32)."""
    x, y, z = (np.asarray(v, np.float32) for v in xyz)
    dx, dy, dz = np.float32(q[0]) - x, np.float32(q[1]) - y, np.float32(q[2]) - z
    d2 = ((np.float32(0.0) + dx * dx) + dy * dy) + dz * dz
    nb = np.flatnonzero(d2 < np.float32(rr))
    nb = nb[np.lexsort((nb, d2[nb]))]
    return nb, d2[nb]


def tie_case(k=320, first=100, seed=700):
    """A blob of k points whose query is its first point.  The neighbours from position `first` of
    the FLANN order on share the normal -d, the nearer ones have 4 d: the normals' sum is a positive
    multiple of d, so z . d >= 0 after the disambiguation and the cosines of the k - first far
    neighbours, spread over several waves and over both chunks, are one float, the minimum, and the
    neighbour at position `first` must win.  Returns the surface, its normals, the query and the winner's row."""
    xyz, _ = C.blob(k, (1.0, 2.0, 3.0), seed)
    q = tuple(v[:1] for v in xyz)
    nb, _ = flann_order(xyz, [v[0] for v in q], C.R * C.R)
    assert len(nb) == k and nb[0] == 0
    d = np.asarray((0.36, 0.48, 0.8))
    n = np.repeat(4.0 * d[None], k, axis=0)
    n[nb[first:]] = -d
    return xyz, f32(n[:, 0], n[:, 1], n[:, 2]), q, nb, first


def random_cloud(n=600, seed=710, side=0.12):
    """n random points in a cube of `side` with random unit normals: neighbourhoods of a few dozen to
    a few hundred points at r = 0.05, for the three tangent radii."""
    p = np.asarray((1.0, 2.0, 3.0)) + np.random.default_rng(seed).uniform(-0.5 * side, 0.5 * side, (n, 3))
    return f32(p[:, 0], p[:, 1], p[:, 2]), C.unit_normals(n, seed + 1)
