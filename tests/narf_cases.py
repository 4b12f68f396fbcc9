"""NARF / range-image cases off the default camera and parameters, shared by the oracle's CPU
tests (test_oracle_narf_params.py) and the GPU parity tests (test_gpu_narf_params.py).

A case is a triple (cloud spec, camera dict, params dict); the dicts hold only what differs from
the defaults (oracle_lib.CAM_DEFAULT / NARF_DEFAULT, pfx_camera_default / pfx_narf_params_default).
The GPU side turns them into camera(**d) and narf_params(**d), the oracle side passes them as they
are.  Clouds and oracle results are computed once per process and handed out read-only.
"""
import functools
import os

import numpy as np

import oracle_lib as O

# The small camera: npx = 19,159 (no multiple of 32 or 64), fx != fy, off-integer centre.
S = dict(width=161, height=119, center_x=80.5, center_y=59.0, focal_length_x=131.25, focal_length_y=140.0)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    r = np.eye(3)
    r[i, i] = c
    r[j, j] = c
    r[i, j] = -s
    r[j, i] = s
    return r


def _pose(r, t):
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = t
    return m


# laser -> camera axis matrix of RangeImage::LASER_FRAME: to_world = sensor_pose * L
L = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float64)

POSES = {
    # 90 degrees about z (entries 0, +-1) and a dyadic translation: to_ri * p is exact on a cloud
    # quantised to 2^-10 m
    "exact90": _pose(np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), [0.5, -0.25, 0.125]),
    "G": _pose(_rot("y", 0.3), [0.1, -0.2, 0.05]),
    # rotation about all three axes, |t| = 1.0 m
    "H": _pose(_rot("z", 0.4) @ _rot("y", -0.35) @ _rot("x", 0.25), [0.7, -0.6, 0.4]),
    # looks along -z: every point of a z > 0 cloud is behind the sensor
    "away": _pose(_rot("y", np.pi), [0.0, 0.0, 0.0]),
}
POSES["GL"] = POSES["G"] @ L


def pose32(name):
    return POSES[name].astype(np.float32)


def _frozen(*arrays):
    out = tuple(np.ascontiguousarray(a, np.float32) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def room_box():
    """The cloud of test_gpu_narf.test_narf_every_region_grow_path: synth_room(40_000, 11) plus a
    small box 0.16-0.5 m in front of the sensor (windows beyond the flood-fill masks and beyond the
    windowed bitmap)."""
    from pcl_feature_extraction_amd.synth import synth_room
    x, y, z, _ = synth_room(40_000, 11)
    rng = np.random.default_rng(12)
    u = rng.uniform(-0.03, 0.03, (3000, 2))
    near = np.c_[u, rng.choice([0.16, 0.5], 3000)].astype(np.float32)
    side = np.c_[np.full(1500, 0.03), rng.uniform(-0.03, 0.03, 1500), rng.uniform(0.16, 0.5, 1500)]
    pts = np.concatenate([np.c_[x, y, z], near, side.astype(np.float32)]).astype(np.float32)
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


@functools.lru_cache(maxsize=None)
def cloud(spec):
    """spec: ("indoor",) the golden cloud indoor_source | ("indoor_q",) the same quantised to
    2^-10 m | ("room_box",) | ("moved", spec, pose name): the pose applied in float64, then cast
    to float32."""
    kind = spec[0]
    if kind == "indoor":
        from pcl_feature_extraction_amd.pcd import read_pcd
        c = read_pcd(os.path.join(os.path.dirname(__file__), "golden", "clouds", "indoor_source.pcd"))
        return _frozen(c.x, c.y, c.z)
    if kind == "indoor_q":
        return _frozen(*(np.round(np.asarray(v, np.float64) * 1024.0) / 1024.0 for v in cloud(("indoor",))))
    if kind == "room_box":
        return _frozen(*room_box())
    if kind == "moved":
        x, y, z = (np.asarray(v, np.float64) for v in cloud(spec[1]))
        m = POSES[spec[2]]
        return _frozen(*(m[i, 0] * x + m[i, 1] * y + m[i, 2] * z + m[i, 3] for i in range(3)))
    raise KeyError(spec)


def _posed(base, name, **cam):
    """The cloud moved by a pose and the camera S at that pose: sees what S sees at identity."""
    return ("moved", (base,), name), dict(S, sensor_pose=pose32(name), **cam)


INDOOR = ("indoor",)
_GL_CLOUD = ("moved", INDOOR, "GL")
_G_LASER = dict(S, sensor_pose=pose32("G"), coordinate_frame=1)

# ---- range image cases: name -> (cloud spec, camera dict) ------------------------------------
RANGE_CASES = {
    "S": (INDOOR, dict(S)),
    "S_exact90": _posed("indoor_q", "exact90"),
    "S_G": _posed("indoor", "G"),
    "S_H": _posed("indoor", "H"),
    "S_G_laser": (_GL_CLOUD, _G_LASER),
    "S_min_range": (INDOOR, dict(S, min_range=1.5)),
    "17x13": (INDOOR, dict(width=17, height=13, center_x=8.0, center_y=6.5, focal_length_x=14.0, focal_length_y=14.5)),
    "1x1": (INDOOR, dict(width=1, height=1, center_x=0.0, center_y=0.0, focal_length_x=1.5, focal_length_y=1.25)),
    "S_away": (INDOOR, dict(S, sensor_pose=pose32("away"))),
}

# ---- the parameter sweep at S, identity pose --------------------------------------------------
# (id, params, first stage whose oracle output differs from the default-parameter run at S);
# None: no stage differs (do_non_maximum_suppression = 0 leaves the 21 keypoints unchanged)
SWEEP = [
    ("prb1", dict(pixel_radius_borders=1), "border_traits"),
    ("prb5", dict(pixel_radius_borders=5), "border_traits"),
    ("prpe0", dict(pixel_radius_plane_extraction=0), "border_traits"),
    # 1 and 3 beside 0 and 4: 0 is degenerate (NO_KEYPOINTS below), and
    # 3 is the radius with the most neighbours per pixel (step 2: 4 x 4 = 16 of k_surface's 25 slots;
    # radius 4 has step 3 and 3 x 3 = 9)
    ("prpe1", dict(pixel_radius_plane_extraction=1), "border_traits"),
    ("prpe3", dict(pixel_radius_plane_extraction=3), "border_traits"),
    ("prpe4", dict(pixel_radius_plane_extraction=4), "border_traits"),
    ("prbd0", dict(pixel_radius_border_direction=0), "surface_change"),
    ("prbd4", dict(pixel_radius_border_direction=4), "surface_change"),
    ("prpc1", dict(pixel_radius_principal_curvature=1), "surface_change"),
    ("prpc4", dict(pixel_radius_principal_curvature=4), "surface_change"),
    ("mbp0.5", dict(minimum_border_probability=0.5), "border_traits"),
    ("min_scs0.05", dict(min_surface_change_score=0.05), "interest"),
    ("opt_dist0.5", dict(optimal_distance_to_high_surface_change=0.5), "interest"),
    ("min_interest0.2", dict(min_interest_value=0.2), "keypoints"),
    ("cap5", dict(max_no_of_interest_points=5), "keypoints"),
    ("min_dist1.0", dict(min_distance_between_interest_points=1.0), "keypoints"),
    ("nms0", dict(do_non_maximum_suppression=0), None),
    # beyond the table: the three radii without a structural bound, well past 3 together and each
    # at narf_dev's limit of 1024 (5 / 1 / 13 oracle keypoints; far larger than the image, so every
    # loop runs off all four edges)
    ("radii8", dict(pixel_radius_borders=8, pixel_radius_border_direction=8, pixel_radius_principal_curvature=8),
     "border_traits"),
    ("prb1024", dict(pixel_radius_borders=1024), "border_traits"),
    ("prbd1024", dict(pixel_radius_border_direction=1024), "surface_change"),
    ("prpc1024", dict(pixel_radius_principal_curvature=1024), "surface_change"),
]

# ---- NARF cases: name -> (cloud spec, camera dict, params dict) ------------------------------
NARF_CASES = {"default": (INDOOR, dict(S), {})}
for _id, _p, _stage in SWEEP:
    NARF_CASES[_id] = (INDOOR, dict(S), _p)
NARF_CASES["min_range1.5"] = (INDOOR, dict(S, min_range=1.5), {})
for _name in ("exact90", "G", "H"):
    NARF_CASES["pose_" + _name] = _posed("indoor_q" if _name == "exact90" else "indoor", _name) + ({},)
NARF_CASES["G_laser"] = (_GL_CLOUD, _G_LASER, {})
for _s in (0.1, 0.5, 1.0):
    NARF_CASES["G_laser_support%g" % _s] = (_GL_CLOUD, _G_LASER, dict(support_size=_s))

# pixel_radius_plane_extraction = 0: one neighbour per pixel (the pixel itself), so
# getSurfaceInformation has fewer than 3 samples everywhere, no pixel gets a normal, every border
# score is 0 and the trait, surface-change and interest images are all zero: no keypoints.  The
# case pins that the GPU agrees on this degenerate path; prpe1 / prpe3 are the non-trivial ones.
NO_KEYPOINTS = {"prpe0"}
# a border-direction window of the whole image averages nearly every direction away: 1 keypoint,
# 531 surface-change scores and 3217 interest values differ from the default run
FEW_KEYPOINTS = {"prbd1024"}

# ---- full size: the posed room with the near-sensor box, and the 1024-wide image ------------
FULL_POSED = (("moved", ("room_box",), "H"), dict(sensor_pose=pose32("H")),
              dict(calculate_sparse_interest_image=0))
WIDE = (INDOOR, dict(width=1024, height=64, center_x=512.0, center_y=32.0, focal_length_x=525.0,
                     focal_length_y=525.0), dict(calculate_sparse_interest_image=0))
NARF_CASES["full_posed"] = FULL_POSED
NARF_CASES["wide1024"] = WIDE
SMALL_CASES = [k for k in NARF_CASES if k not in ("full_posed", "wide1024")]


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_range(name):
    spec, cam = RANGE_CASES[name]
    return _ro(O.range_image_planar(*cloud(spec), cam=cam))


@functools.lru_cache(maxsize=None)
def oracle_narf(name):
    """(keypoints, dict(interest, surface_change, border_traits, range)) of the oracle: the complete
    interest formula, whatever the case says about calculate_sparse_interest_image."""
    spec, cam, params = NARF_CASES[name]
    p = {k: v for k, v in params.items() if k != "calculate_sparse_interest_image"}
    kp, dbg = O.narf_keypoints(*cloud(spec), params=p, cam=cam, debug=True)
    dbg["range"] = O.range_image_planar(*cloud(spec), cam=cam)[..., 3].copy()
    for v in dbg.values():
        _ro(v)
    return _ro(kp), dbg
