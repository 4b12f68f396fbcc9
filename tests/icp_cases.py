"""Clouds of the ICP tests, shared by the restatement's analytic cases (test_icp_ref.py) and the
GPU comparison (test_gpu_icp.py).  Every case is (source xyz, target xyz, params, guess); params
update icp_ref.REFERENCE."""
import numpy as np

F = np.float32


def lattice(m, spacing=0.1, jitter=0.01, seed=0):
    """m^3 jittered lattice points as (x, y, z) float32: neighbours are at least spacing - 2 jitter
    apart."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    p = g * spacing + rng.uniform(-jitter, jitter, g.shape)
    p = p[rng.permutation(len(p))]  # index order unrelated to position
    return tuple(np.ascontiguousarray(p[:, i], F) for i in range(3))


DELTA = np.array([0.02, -0.015, 0.01])  # |delta| = 0.027 < half the lattice's 0.08 minimum spacing


def shifted(tgt, delta=DELTA):
    """source = target - delta in float: the aligning translation is delta."""
    return tuple((v - F(d)).astype(F) for v, d in zip(tgt, delta))


def identical():
    t = lattice(7, seed=1)
    return tuple(v.copy() for v in t), t, {}, None


def shifted_lattice():
    """n = 512; aligned after one step, TRANSFORM at the second."""
    t = lattice(8, seed=2)
    return shifted(t), t, {}, None


def far_apart():
    t = lattice(5, seed=3)
    s = (t[0] + F(10.0), t[1].copy(), t[2].copy())
    return s, t, {}, None


def one_iteration():
    s, t, _, _ = shifted_lattice()
    return s, t, dict(max_iterations=1), None


def ties():
    """Source points with two target points at exactly the same d2 (mirror images across the
    source point, and a duplicated target point): the lower target index must win, and which
    mirror image wins moves the fit."""
    tx, ty, tz, sx, sy, sz = [], [], [], [], [], []
    for k in range(6):
        c = (0.5 * k, 0.25 * (k % 3), 0.125 * (k % 2))  # exact in float, as are c +- 1/32
        a = 0.03125
        first = a if k % 2 else -a  # the lower index alternates between the two sides
        tx += [c[0] + first, c[0] - first]
        ty += [c[1], c[1]]
        tz += [c[2], c[2]]
        sx.append(c[0]); sy.append(c[1]); sz.append(c[2])
    # a duplicated target point (indices 12 and 13) with its source point
    tx += [3.5, 3.5]; ty += [1.0, 1.0]; tz += [0.5, 0.5]
    sx.append(3.5 + 0.015625); sy.append(1.0); sz.append(0.5)
    arr = lambda v: np.asarray(v, F)  # noqa: E731
    return (arr(sx), arr(sy), arr(sz)), (arr(tx), arr(ty), arr(tz)), dict(max_iterations=1), None


def exact_cap():
    """Distance cap 0.5: source 0 lies at exactly d2 = 0.25 from its target (kept), source 1 at the
    next float above (dropped); four exact matches complete the list."""
    up = np.nextafter(F(0.5), F(1.0))
    tx = [0.0, 0.0, 4.0, 8.0, 4.0, 8.0]
    ty = [0.0, 10.0, 0.0, 0.0, 6.0, 6.0]
    tz = [0.0, 0.0, 1.0, 2.0, 3.0, 5.0]
    sx = [0.5, up] + tx[2:]
    arr = lambda v: np.asarray(v, F)  # noqa: E731
    return (arr(sx), arr(ty), arr(tz)), (arr(tx), arr(ty), arr(tz)), dict(max_correspondence_distance=0.5,
                                                                     max_iterations=1), None


def with_nans():
    """shifted_lattice with non-finite points in both clouds; second value: the same clouds with
    those points removed."""
    s, t, p, g = shifted_lattice()
    s = [v.copy() for v in s]
    t = [v.copy() for v in t]
    bad_s, bad_t = [3, 100, 101, 511], [0, 7, 300]
    s[0][3] = np.nan; s[1][100] = np.inf; s[2][101] = np.nan; s[0][511] = -np.inf
    t[2][0] = np.nan; t[0][7] = np.inf; t[1][300] = np.nan
    ks = np.setdiff1d(np.arange(512), bad_s)
    kt = np.setdiff1d(np.arange(512), bad_t)
    clean = (tuple(v[ks] for v in s), tuple(v[kt] for v in t), p, g)
    return (tuple(s), tuple(t), p, g), clean


def list_length(n_list, seed=11):
    """Exactly n_list source points have a target point within the cap; 37 more, scattered among
    them, have none."""
    m = 3
    while m ** 3 < n_list + 20:
        m += 1
    t = lattice(m, seed=seed)
    rng = np.random.default_rng(seed + 1)
    near = shifted(tuple(v[:n_list] for v in t), DELTA * 0.5)
    far = (rng.uniform(-3.0, -2.0, 37), rng.uniform(5.0, 6.0, 37), rng.uniform(0.0, 1.0, 37))
    s = np.concatenate([np.stack(near, 1), np.stack(far, 1).astype(F)])
    s = s[rng.permutation(len(s))]
    return tuple(np.ascontiguousarray(s[:, i], F) for i in range(3)), t, {}, None


def retry_rounds():
    """Sparse target (spacing 0.3) and cap 0.5: the first grid (cell about 0.15) certifies only
    the close pairs; pairs 0.17 apart need the second grid, pairs 0.4 apart the third, and points
    2 away are certified to have no correspondence there."""
    t = lattice(5, spacing=0.3, jitter=0.0, seed=4)
    k = len(t[0])
    off = np.zeros((k, 3))
    off[0::4] = (0.01, 0.0, 0.0)
    off[1::4] = (0.12, 0.12, 0.0)
    off[2::4] = (0.005, -0.01, 0.0)
    off[3::4] = (0.0, 0.01, 0.012)
    s = np.stack(t, 1).astype(np.float64) + off
    lo = np.stack(t, 1).min(0)
    outside = np.array([[lo[0] - 0.4, lo[1] + 0.3, lo[2] + 0.3], [lo[0] + 0.6, lo[1] - 0.4, lo[2] + 0.6],
                        [lo[0] - 2.0, lo[1], lo[2]], [lo[0] + 0.3, lo[1] + 0.3, lo[2] + 3.2]])
    s = np.concatenate([s, outside])
    return tuple(np.ascontiguousarray(s[:, i], F) for i in range(3)), t, dict(max_correspondence_distance=0.5), None


def default_distance(pcl_default):
    """PCL's default parameters (no effective cap) on 300 target points; 6 source points lie far
    outside every grid and fall to the exhaustive scan."""
    t = tuple(v[:300] for v in lattice(7, seed=5))
    s = np.stack(shifted(t, DELTA * 0.3), 1).astype(np.float64)[:280]
    far = np.array([[6.0, 0.2, 0.1], [-5.0, 0.3, 0.3], [0.3, 7.0, 0.2], [0.1, 0.2, -6.5], [5.0, 5.0, 5.0],
                    [-4.0, 4.5, 0.0]])
    s = np.concatenate([s[:100], far[:3], s[100:], far[3:]])
    return tuple(np.ascontiguousarray(s[:, i], F) for i in range(3)), t, dict(pcl_default), None


def with_guess():
    """shifted_lattice seen from a pose 0.02 rad and (0.01, 0.02, -0.015) away; the guess undoes
    most of it."""
    s, t, _, _ = shifted_lattice()
    c, sn = np.cos(0.02), np.sin(0.02)
    G = np.array([[c, -sn, 0, 0.01], [sn, c, 0, 0.02], [0, 0, 1, -0.015], [0, 0, 0, 1]], np.float64)
    Gi = np.linalg.inv(G)
    p = np.stack(s, 1).astype(np.float64) @ Gi[:3, :3].T + Gi[:3, 3]
    return tuple(np.ascontiguousarray(p[:, i], F) for i in range(3)), t, {}, G.astype(F)
