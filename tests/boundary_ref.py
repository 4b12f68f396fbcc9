"""Thin ctypes wrapper around tests/cpp/boundary_ref.cpp, the CPU restatement of PCL 1.7
BoundaryEstimation as DESIGN.md "Boundary: the contract" states it (test infrastructure: nothing under
pcl_feature_extraction_amd/ uses it)."""
import collections
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "boundary_ref.cpp")

_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)

#: flags (nq,) uint8 (0, 1, 255); neighbors / kmax / flagged: the sum and the largest of k and the
#: number of 1s; k: every row's neighbour count; max_gap: the largest gap PCL compares with the
#: threshold (NaN where the row has no angle)
Result = collections.namedtuple("Result", "flags neighbors kmax flagged k max_gap")


def build(out_dir):
    """Compile boundary_ref.cpp into out_dir (the oracle's floating-point contract: -O2, no FMA
    contraction, plain x86-64) and load it."""
    so = os.path.join(str(out_dir), "libboundary_ref.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wl,-z,defs", SRC, "-o", so]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(so)
    lib.boundary_ref.restype = None
    lib.boundary_ref.argtypes = ([_f32p] * 3 + [ctypes.c_int64] + [_f32p] * 6 +
                                 [ctypes.c_int64, ctypes.c_double, ctypes.c_float, _u8p, _i64p, _i64p, _f32p])
    return lib


def _p(v):
    return v.ctypes.data_as(_f32p)


def flags(lib, sx, sy, sz, qx, qy, qz, qnx, qny, qnz, r, angle_threshold=math.pi / 2):
    """The boundary flags of the queries, whose normals are (qnx, qny, qnz)."""
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (sx, sy, sz, qx, qy, qz, qnx, qny, qnz)]
    ns, nq = len(a[0]), len(a[3])
    assert len(a[6]) == nq
    out = np.empty(nq, np.uint8)
    stats, k, gap = np.zeros(3, np.int64), np.zeros(nq, np.int64), np.zeros(nq, np.float32)
    lib.boundary_ref(*map(_p, a[:3]), ns, *map(_p, a[3:]), nq, float(r), float(angle_threshold),
                     out.ctypes.data_as(_u8p), stats.ctypes.data_as(_i64p), k.ctypes.data_as(_i64p), _p(gap))
    return Result(out, int(stats[0]), int(stats[1]), int(stats[2]), k, gap)
