"""Small synthetic inputs of the intensity-spin tests (plain numpy, no GPU), for the search radius R.
Surfaces are (x, y, z) float32 tuples, intensities float32 arrays."""
import math

import numpy as np

import list_edge_clouds as E  # noqa: F401  (the exact-k blobs of the pass boundary and the capacity)
import pfh_cases as C
from rift_cases import NAN_BITS, blobs_case, intensities, order_case  # noqa: F401
from spin_cases import Q0, R, STEP, f32, offset, points  # noqa: F401  (offsets by powers of two: exact)

FAR = (9.0e3, 9.0e3, 9.0e3)


def lone(intensity=7.0):
    """One point, its own centre: d = 0, max == min, i = 0."""
    return points(Q0), np.float32([intensity])


def pair(i_centre=10.0, i_other=30.0, step=(STEP, 0.0, 0.0)):
    """The centre Q0 (row 0) and one neighbour at Q0 + step.  With step = (STEP, 0, 0) and D = 4:
    d = 4 * 2^-6 / (R + eps), about 1.25; with two distinct intensities the darker has i = 0 and the
    brighter i = I exactly (20 + FLT_EPSILON rounds to 20)."""
    return points(Q0, offset(*step)), np.float32([i_centre, i_other])


def pair_d(D=4, r=R):
    """d of pair()'s neighbour, in float32 as the contract forms it."""
    return (np.float32(D) * np.sqrt(np.float32(STEP * STEP))) / (np.float32(r) + np.finfo(np.float32).eps)


def gauss_image(contribs, D=4, I=5, sigma=1.0):  # noqa: E741
    """The image of neighbours at (d, i), in double from math.exp: bin[dj * I + ii]."""
    out = np.zeros(D * I)
    t = 3.0 * sigma
    for d, i in contribs:
        for dj in range(max(math.floor(d - t), 0), min(math.ceil(d + t), D - 1) + 1):
            for ii in range(max(math.floor(i - t), 0), min(math.ceil(i + t), I - 1) + 1):
                out[dj * I + ii] += math.exp(-((d - dj) ** 2 + (i - ii) ** 2) / (2.0 * sigma * sigma))
    return out


def ramp_blob(k=256, seed=610):
    """A blob of k points (each sees all k) whose intensities are a shuffle of 0 .. k - 1: one
    brightest neighbour, with i == I exactly for k - 1 = 255 (255 + FLT_EPSILON rounds to 255)."""
    xyz, _ = C.blob(k, Q0, seed)
    inten = np.random.default_rng(seed + 1).permutation(k).astype(np.float32)
    return xyz, inten


def constant_blob(k=40, value=128.0, seed=620):
    xyz, _ = C.blob(k, Q0, seed)
    return xyz, np.full(k, value, np.float32)


def tile_of(ctx, D, I):  # noqa: E741
    """The neighbours whose weights the kernel forms at once for a D x I image (pfx.h)."""
    return min(256, ctx.stat("ispin_tile_words") // ((D * I) | 1))
