"""Thin ctypes wrapper around tests/cpp/narf_desc_ref.cpp, the CPU restatement of PCL 1.7's NARF
descriptor and of Tools::getIndices as DESIGN.md "NARF descriptors: the contract" states them (test
infrastructure: nothing under pcl_feature_extraction_amd/ uses it).  The range image is the oracle's
(oracle_lib.range_image_planar), or one a test writes by hand."""
import collections
import ctypes
import os
import subprocess

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "narf_desc_ref.cpp")

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)

STATS = ("rows", "invalid_pixels", "pose_failed", "fallback_normals", "ring_max", "background_cells")

#: desc (m, 36), pose (m, 12), keypoint (m,), rot (m,): the rotation of each row; stats: dict over
#: STATS; patch (nk, 10, 10) after step 4 and blur (nk, 20, 20), NaN where the entry gave no patch
Result = collections.namedtuple("Result", "desc pose keypoint rot stats patch blur")


def build(out_dir):
    """Compile narf_desc_ref.cpp into out_dir (the oracle's floating-point contract: -O2, no FMA
    contraction, plain x86-64) and load it."""
    so = os.path.join(str(out_dir), "libnarf_desc_ref.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-Wl,-z,defs", "-I",
           os.path.join(ROOT, "oracle"), SRC, "-o", so]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(so)
    lib.narf_desc_ref.restype = None
    lib.narf_desc_ref.argtypes = ([_f32p, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 4 +
                                  [_f32p, ctypes.c_int, _i32p, ctypes.c_int64, ctypes.c_float, ctypes.c_int, _f32p,
                                   _f32p, _i32p, _f32p, _i64p, _i64p, _f32p, _f32p])
    lib.point_indices_ref.restype = ctypes.c_int64
    lib.point_indices_ref.argtypes = [_f32p] * 3 + [ctypes.c_int64] + [_f32p] * 3 + [ctypes.c_int64, ctypes.c_float,
                                                                                 _i32p, ctypes.c_int64]
    lib.narf_rotations_ref.restype = ctypes.c_int
    lib.narf_rotations_ref.argtypes = [_f32p] * 3
    lib.narf_patch_descriptor_ref.restype = None
    lib.narf_patch_descriptor_ref.argtypes = [_f32p, ctypes.c_float, ctypes.c_float, _f32p, _f32p]
    return lib


def _p(v, t=_f32p):
    return v.ctypes.data_as(t)


def on_image(lib, ri, pixel_idx, support=0.2, rotation_invariant=True, cam=None, debug=False):
    """The descriptors of pixel_idx on the range image ri ((h, w, 4): x, y, z, range)."""
    c, pose = O._cam(cam)
    ri = np.ascontiguousarray(ri, np.float32)
    assert ri.shape == (c["height"], c["width"], 4)
    pix = np.ascontiguousarray(pixel_idx, np.int32)
    nk = len(pix)
    desc, rows_pose = np.empty((5 * nk, 36), np.float32), np.empty((5 * nk, 12), np.float32)
    key, rot = np.empty(5 * nk, np.int32), np.empty(5 * nk, np.float32)
    n_out, stats = np.zeros(1, np.int64), np.zeros(6, np.int64)
    patch = np.empty((nk, 10, 10), np.float32) if debug else None
    blur = np.empty((nk, 20, 20), np.float32) if debug else None
    lib.narf_desc_ref(_p(ri), c["width"], c["height"], c["center_x"], c["center_y"], c["focal_length_x"],
                      c["focal_length_y"], _p(pose), c["coordinate_frame"], _p(pix, _i32p), nk, float(support),
                      int(bool(rotation_invariant)), _p(desc), _p(rows_pose), _p(key, _i32p), _p(rot), _p(n_out, _i64p),
                      _p(stats, _i64p), _p(patch) if debug else None, _p(blur) if debug else None)
    m = int(n_out[0])
    return Result(desc[:m].copy(), rows_pose[:m].copy(), key[:m].copy(), rot[:m].copy(),
                  dict(zip(STATS, map(int, stats))), patch, blur)


def descriptors(lib, x, y, z, pixel_idx, support=0.2, rotation_invariant=True, cam=None, debug=False):
    """The descriptors of pixel_idx on the planar range image of the cloud (the oracle's)."""
    return on_image(lib, O.range_image_planar(x, y, z, cam=cam), pixel_idx, support, rotation_invariant, cam, debug)


def rotations(lib, d0):
    """getRotations of a descriptor at rotation 0: (the rotations in the order chosen, the 36 scores)."""
    d0 = np.ascontiguousarray(d0, np.float32)
    assert d0.shape == (36,)
    rot, score = np.empty(5, np.float32), np.empty(36, np.float32)
    n = lib.narf_rotations_ref(_p(d0), _p(rot), _p(score))
    return rot[:n].copy(), score


def patch_descriptor(lib, patch, support, rho=0.0):
    """Steps 5 and 6 on a 10 x 10 patch: (the 20 x 20 blurred patch, the 36 floats)."""
    patch = np.ascontiguousarray(patch, np.float32)
    assert patch.shape == (10, 10)
    blur, d = np.empty((20, 20), np.float32), np.empty(36, np.float32)
    lib.narf_patch_descriptor_ref(_p(patch), float(support), float(rho), _p(blur), _p(d))
    return blur, d


def point_indices(lib, x, y, z, kx, ky, kz, tol=1e-4):
    a = [np.ascontiguousarray(v, np.float32) for v in (x, y, z, kx, ky, kz)]
    n, nk = len(a[0]), len(a[3])
    m = lib.point_indices_ref(*map(_p, a[:3]), n, *map(_p, a[3:]), nk, float(tol), None, 0)
    out = np.empty(max(int(m), 1), np.int32)
    lib.point_indices_ref(*map(_p, a[:3]), n, *map(_p, a[3:]), nk, float(tol), _p(out, _i32p), int(m))
    return out[:m].copy()
