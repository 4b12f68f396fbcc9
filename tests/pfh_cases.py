"""Small synthetic inputs of the PFH tests (plain numpy, no GPU): every builder returns
((x, y, z), (nx, ny, nz)) float32 surface arrays, for the search radius R."""
import numpy as np

R = 0.05


def _f32(*a):
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in a)


def plane_patch(side=9, spacing=0.005, extra=()):
    """side x side points on z = 1.0f exactly, distinct (x, y), all normals (0, 0, 1): every pair
    has f1 = f2 = f3 = 0, i.e. bin 2 + 5 * 2 + 25 * 2 = 62.  The patch spans
    (side - 1) * spacing * sqrt(2) < R, so its centre point (row side * side // 2) sees all of it.
    extra: further (x, y) points appended after the grid."""
    i = np.arange(side)
    gx, gy = np.meshgrid(i, i, indexing="ij")
    xy = np.stack([0.5 + gx.ravel() * spacing, 0.25 + gy.ravel() * spacing], 1)
    if len(extra):
        xy = np.concatenate([xy, np.asarray(extra, np.float64)])
    n = len(xy)
    xyz = _f32(xy[:, 0], xy[:, 1], np.ones(n))
    assert len({(a, b) for a, b in zip(xyz[0].tolist(), xyz[1].tolist())}) == n
    return xyz, _f32(np.zeros(n), np.zeros(n), np.ones(n))


def lattice_patch(dims=(6, 6, 3), spacing=0.01, normal=(0.36, 0.48, 0.8), seed=7):
    """An integer lattice (the same coordinate values on every axis, so many pairs of a
    neighbourhood have bit-equal d2) with one normal for every point and shuffled point indices:
    angle1 == angle2 for every pair, so the swap test never fires and which point is p1 -- the
    later one in (d2, index) order -- decides the sign of f3."""
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    g = g[np.random.default_rng(seed).permutation(len(g))]
    p = (g * spacing).astype(np.float32)
    n = len(p)
    nrm = np.repeat(np.asarray(normal, np.float32)[None], n, axis=0)
    return _f32(p[:, 0], p[:, 1], p[:, 2]), _f32(nrm[:, 0], nrm[:, 1], nrm[:, 2])


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return _f32(v[:, 0], v[:, 1], v[:, 2])


def blob(k, centre, seed, side=0.025):
    """k random points in a cube whose diagonal is below R (each sees all k) + unit normals."""
    p = np.asarray(centre) + np.random.default_rng(seed).uniform(-0.5 * side, 0.5 * side, (k, 3))
    return _f32(p[:, 0], p[:, 1], p[:, 2]), unit_normals(k, seed + 1)


def concat(parts):
    """[((x, y, z), (nx, ny, nz))] -> one surface and the (first, end) rows of every part."""
    rows, at = [], 0
    for xyz, _ in parts:
        rows.append((at, at + len(xyz[0])))
        at += len(xyz[0])
    xyz = tuple(np.concatenate([p[0][a] for p in parts]) for a in range(3))
    nrm = tuple(np.concatenate([p[1][a] for p in parts]) for a in range(3))
    return xyz, nrm, rows
