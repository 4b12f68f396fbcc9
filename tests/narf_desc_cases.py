"""NARF descriptor cases shared by the restatement's CPU tests (test_narf_desc_ref.py) and the GPU
parity tests (test_gpu_narf_desc.py): synthetic scenes small enough to reason about, and the golden
indoor cloud at the cameras of narf_cases.py.  Clouds, range images and pixel lists are computed once
per process and handed out read-only."""
import functools

import numpy as np

import narf_cases as NC
import oracle_lib as O

S = NC.S
FULL = dict(O.CAM_DEFAULT)
del FULL["sensor_pose"]


def _ro(a):
    a.setflags(write=False)
    return a


# ---- synthetic range images ------------------------------------------------------------------
# A small pinhole camera at the origin looking along +z, centre on a pixel so that the central ray is
# the optical axis: a fronto-parallel wall through (0, 0, d) has its normal along the view direction.
T = dict(width=81, height=61, center_x=40.0, center_y=30.0, focal_length_x=100.0, focal_length_y=100.0)
T_CENTRE = 30 * 81 + 40


def depth_image(depth, cam=T):
    """The range image ((h, w, 4) float32: x, y, z, range) of a depth map z(v, u) (NaN / +-inf: no
    return): every pixel's point lies on its own ray, as calculate3DPoint puts it there."""
    h, w = cam["height"], cam["width"]
    depth = np.broadcast_to(np.asarray(depth, np.float64), (h, w))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dx, dy = (u - cam["center_x"]) / cam["focal_length_x"], (v - cam["center_y"]) / cam["focal_length_y"]
    ok = np.isfinite(depth)
    z = np.where(ok, depth, np.nan)
    out = np.stack([dx * z, dy * z, z, z * np.sqrt(dx * dx + dy * dy + 1.0)], -1).astype(np.float32)
    out[~ok, 3] = -np.inf
    return out


def plane_depth(n, d, cam=T):
    """Depth map of the plane n . p = n . (0, 0, d) seen by the camera (every pixel hits it)."""
    h, w = cam["height"], cam["width"]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dx, dy = (u - cam["center_x"]) / cam["focal_length_x"], (v - cam["center_y"]) / cam["focal_length_y"]
    n = np.asarray(n, np.float64)
    return n[2] * d / (n[0] * dx + n[1] * dy + n[2])


# The finer camera of the relief scenes: a pixel is 5 mm at 2 m, a quarter of a patch cell of the
# support 0.2; square pixels and the centre on a pixel, so a quarter turn of the depth map about the
# centre pixel is a quarter turn of the scene about the optical axis.
Q = dict(width=65, height=65, center_x=32.0, center_y=32.0, focal_length_x=400.0, focal_length_y=400.0)
Q_CENTRE = 32 * 65 + 32


def relief_depth(height, cam=Q, d=2.0):
    """Depth map of the surface z = d - height (x, y) (a relief towards the sensor on the wall z = d),
    by fixed-point iteration along every pixel's ray."""
    h, w = cam["height"], cam["width"]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dx, dy = (u - cam["center_x"]) / cam["focal_length_x"], (v - cam["center_y"]) / cam["focal_length_y"]
    z = np.full_like(dx, d)
    for _ in range(40):
        z = d - height(dx * z, dy * z)
    return z


def groove_depth(half_width=0.04, delta=0.03, cam=Q, d=2.0):
    """The wall z = d for |x| < half_width, z = d + delta beyond: even in x and y, so the pose stays
    upright and every beam that leaves the strip crosses one step of height delta."""
    w = cam["width"]
    dx = (np.arange(w, dtype=np.float64) - cam["center_x"]) / cam["focal_length_x"]
    return np.broadcast_to(np.where(np.abs(dx * d) < half_width, d, d + delta), (cam["height"], w))


def square_depth(behind, half=0.045, cam=Q, d=2.0):
    """A square of side 2 half at z = d, and `behind` (a depth, or NaN for nothing) around it."""
    h, w = cam["height"], cam["width"]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dx, dy = (u - cam["center_x"]) / cam["focal_length_x"], (v - cam["center_y"]) / cam["focal_length_y"]
    return np.where((np.abs(dx * d) <= half) & (np.abs(dy * d) <= half), d, behind)


def x_ridge(x, y):
    """Two ridges of height 0.02 and half-width 0.015 along the diagonals: four-fold symmetric."""
    return 0.02 * np.maximum(0.0, 1.0 - np.minimum(np.abs(x - y), np.abs(x + y)) / (np.sqrt(2.0) * 0.015))


def even_relief(x, y):
    """Four bumps, point-symmetric about the keypoint (so the weighted covariance has no xz or yz term
    and the normal stays the optical axis) but with no quarter-turn symmetry."""
    def g(a, b, s):
        return np.exp(-((x - a) ** 2 + (y - b) ** 2) / (2 * s * s))
    return 0.02 * (g(0.045, 0.012, 0.02) + g(-0.045, -0.012, 0.02)) + 0.01 * (g(-0.02, 0.05, 0.015) + g(0.02, -0.05, 0.015))


def turned(height, phi):
    """The relief `height` turned by +phi about the optical axis through the keypoint (x towards y)."""
    c, s = np.cos(phi), np.sin(phi)
    return lambda x, y: height(c * x + s * y, -s * x + c * y)


def image_cloud(ri):
    """The valid pixels' points as a cloud: projected again they fall on their own pixels."""
    ok = np.isfinite(ri[..., 3])
    p = ri[ok]
    return tuple(np.ascontiguousarray(p[:, i]) for i in range(3))


# ---- the indoor cloud -----------------------------------------------------------------------
def _lonely_points(ri, cam, count):
    """Points that land exactly on pixels whose 7 x 7 window the scan left empty, at z = 525 / 256 (with
    camera S the products below are exact, so floor = ceil = round and one pixel is filled): each
    has no neighbour at all, the pose fails."""
    valid = np.isfinite(ri[..., 3])
    h, w = valid.shape
    z = 525.0 / 256.0
    out, taken = [], np.zeros_like(valid)
    for py in range(4, h - 4):
        for px in range(4, w - 4):
            if valid[py - 3:py + 4, px - 3:px + 4].any() or taken[max(0, py - 6):py + 7, max(0, px - 6):px + 7].any():
                continue
            m, j = px - 81, py - 59
            out.append(((2 * m + 1) / 128.0, 15.0 * j / 1024.0, z))
            taken[py, px] = True
            if len(out) == count:
                return np.array(out, np.float32), np.flatnonzero(taken.ravel()).astype(np.int32)
    raise AssertionError("no empty windows in the range image")


@functools.lru_cache(maxsize=None)
def indoor(name):
    """(x, y, z, camera dict, pixel_idx) of a named case on the golden indoor cloud.  pixel_idx: the
    case's NARF keypoints, then a lattice of every 7th pixel (invalid pixels and image-edge patches
    among them), then one negative index and one beyond the image."""
    if name == "lonely":  # the base cloud plus 6 points with empty surroundings, listed first
        x, y, z, cam, pix = indoor("S")
        ri = O.range_image_planar(x, y, z, cam=cam)
        pts, at = _lonely_points(ri, cam, 6)
        x, y, z = (np.concatenate([a, pts[:, i]]) for i, a in enumerate((x, y, z)))
        return _ro(x), _ro(y), _ro(z), cam, _ro(np.concatenate([at, pix]))
    if name == "full":  # 640 x 480: 64 entries over the whole index range
        x, y, z = NC.cloud(NC.INDOOR)
        npx = FULL["width"] * FULL["height"]
        ri = O.range_image_planar(x, y, z, cam=FULL)
        valid = np.flatnonzero(np.isfinite(ri[..., 3].ravel()))
        pick = valid[np.linspace(0, len(valid) - 1, 60).astype(np.int64)]
        pix = np.concatenate([pick, [valid[-1], npx - 1, 0, npx]]).astype(np.int32)
        return x, y, z, dict(FULL), _ro(pix)
    case = {"S": "default", "H": "pose_H", "laser": "G_laser"}[name]
    spec, cam, _ = NC.NARF_CASES[case]
    x, y, z = NC.cloud(spec)
    kp, _ = NC.oracle_narf(case)
    npx = cam["width"] * cam["height"]
    pix = np.concatenate([kp.astype(np.int32), np.arange(0, npx, 7, dtype=np.int32), np.array([-1, npx], np.int32)])
    return x, y, z, dict(cam), _ro(pix)


#: (case of indoor(), support_size, rotation_invariant, what the restatement must reach there)
GPU_CASES = [
    ("S", 0.2, True, ("multi", "fallback", "background")),
    ("S", 0.2, False, ("fallback", "background")),
    ("S", 1.0, True, ("multi", "background", "rings")),
    ("lonely", 0.02, True, ("multi", "fallback", "failed", "background")),
    ("H", 0.2, True, ("multi", "background")),
    ("laser", 0.2, True, ("multi", "background")),
    ("full", 0.2, True, ("multi", "background", "rings")),
]
