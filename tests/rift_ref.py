"""Thin ctypes wrapper around tests/cpp/rift_ref.cpp, the CPU restatements of the intensity gradient
(float accessor) and of PCL 1.7 RIFTEstimation (test infrastructure: nothing under
pcl_feature_extraction_amd/ uses it), and a direct Python statement of Eigen 3.2's float summation
order."""
import collections
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rift_ref.cpp")

_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)

#: out (nq, 3) or (nq, D G) float32, then the counts
Result = collections.namedtuple("Result", "out neighbors kmax")


def build(out_dir):
    """Compile rift_ref.cpp into out_dir (the oracle's floating-point contract: -O2, no FMA
    contraction, plain x86-64) and load it."""
    so = os.path.join(str(out_dir), "librift_ref.so")
    oracle = os.path.join(ROOT, "oracle")
    # (the oracle's ColPivHouseholderQR restatement lives in or_keypoints.cpp, which calls or_features.cpp)
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wl,-z,defs", "-I", oracle, SRC,
           os.path.join(oracle, "or_keypoints.cpp"), os.path.join(oracle, "or_features.cpp"), "-o", so]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(so)
    lib.igrad_ref.restype = None
    lib.igrad_ref.argtypes = ([_f32p] * 4 + [ctypes.c_int64] + [_f32p] * 6 +
                              [ctypes.c_int64, ctypes.c_double, ctypes.c_int, _f32p, _i64p])
    lib.rift_ref.restype = None
    lib.rift_ref.argtypes = ([_f32p] * 6 + [ctypes.c_int64] + [_f32p] * 3 +
                             [ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p, _i64p])
    lib.rift_eigen_sum_f.restype = ctypes.c_float
    lib.rift_eigen_sum_f.argtypes = [_f32p, ctypes.c_int]
    return lib


def _arrs(*a):
    return [np.ascontiguousarray(v, dtype=np.float32) for v in a]


def _p(v):
    return v.ctypes.data_as(_f32p)


def gradient(lib, sx, sy, sz, si, qx, qy, qz, qnx, qny, qnz, r, reversed_order=False):
    """The intensity gradient's rows, (nq, 3)."""
    a = _arrs(sx, sy, sz, si, qx, qy, qz, qnx, qny, qnz)
    ns, nq = len(a[0]), len(a[4])
    out = np.empty((nq, 3), np.float32)
    stats = np.zeros(2, np.int64)
    lib.igrad_ref(*map(_p, a[:4]), ns, *map(_p, a[4:]), nq, float(r), 1 if reversed_order else 0, _p(out),
                  stats.ctypes.data_as(_i64p))
    return Result(out, int(stats[0]), int(stats[1]))


def rift(lib, sx, sy, sz, sgx, sgy, sgz, cx, cy, cz, r, nr_distance_bins=4, nr_gradient_bins=8, reversed_order=False):
    """RIFT's rows, (nq, D G): row[gi * D + di]."""
    a = _arrs(sx, sy, sz, sgx, sgy, sgz, cx, cy, cz)
    ns, nq = len(a[0]), len(a[6])
    out = np.empty((nq, nr_distance_bins * nr_gradient_bins), np.float32)
    stats = np.zeros(2, np.int64)
    lib.rift_ref(*map(_p, a[:6]), ns, *map(_p, a[6:]), nq, float(r), int(nr_distance_bins), int(nr_gradient_bins),
                 1 if reversed_order else 0, _p(out), stats.ctypes.data_as(_i64p))
    return Result(out, int(stats[0]), int(stats[1]))


def eigen_sum(lib, m):
    m = np.ascontiguousarray(m, dtype=np.float32)
    return np.float32(lib.rift_eigen_sum_f(_p(m), len(m)))


def eigen_sum_py(m):
    """Eigen 3.2's sum() of a float array, from Redux.h (SSE packets of four floats, two accumulators):
    eight running sums over the indices mod 8 below 8 * (S // 8), combined lane-wise to four; one more
    packet added lane-wise when 4 * (S // 4) > 8 * (S // 8); predux (a0 + a2) + (a1 + a3); the scalar tail
    added left to right.  (No packet at all, S < 4: sequential.)"""
    m = [np.float32(v) for v in m]
    S = len(m)
    if S == 0:
        return np.float32(0.0)
    if S < 4:
        res = m[0]
        for v in m[1:]:
            res = res + v
        return res
    end4, end8 = 4 * (S // 4), 8 * (S // 8)
    a = m[:4]
    if end8:
        s = m[:8]
        for i in range(8, end8):
            s[i % 8] = s[i % 8] + m[i]
        a = [s[lane] + s[lane + 4] for lane in range(4)]
        if end4 > end8:
            a = [a[lane] + m[end8 + lane] for lane in range(4)]
    res = (a[0] + a[2]) + (a[1] + a[3])
    for v in m[end4:]:
        res = res + v
    return res


def sequential_sum(m):
    res = np.float32(0.0)
    for v in m:
        res = res + np.float32(v)
    return res
