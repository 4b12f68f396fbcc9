"""Thin ctypes wrapper around tests/cpp/spin_ref.cpp, the CPU restatement of PCL 1.7
SpinImageEstimation (test infrastructure: nothing under pcl_feature_extraction_amd/ uses it), and a
direct Python statement of Eigen 3.2's summation order."""
import collections
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "spin_ref.cpp")

_f32p = ctypes.POINTER(ctypes.c_float)
_f64p = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)

#: out (nq, S) float32, raw (nq, S) float64, sums (nq,) float64, then the counts
Result = collections.namedtuple("Result", "out raw sums neighbors kmax too_few bad_cos first_few first_bad")


def size(w):
    return (w + 1) * (2 * w + 1)


def build(out_dir):
    """Compile spin_ref.cpp into out_dir (the oracle's floating-point contract: -O2, no FMA
    contraction, plain x86-64) and load it."""
    so = os.path.join(str(out_dir), "libspin_ref.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"),
           SRC, "-o", so]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(so)
    lib.spin_ref.restype = ctypes.c_int
    lib.spin_ref.argtypes = ([_f32p] * 6 + [ctypes.c_int64] + [_f32p] * 6 +
                             [ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                              _f32p, _f64p, _f64p, _i64p])
    lib.spin_eigen_sum.restype = ctypes.c_double
    lib.spin_eigen_sum.argtypes = [_f64p, ctypes.c_int]
    return lib


def spin(lib, sx, sy, sz, qx, qy, qz, ax, ay, az, r, image_width=8, support_angle_cos=0.0, min_pts_neighb=0,
         surface_normals=None, reversed_order=False):
    """The restatement's rows; an offending row (too few neighbours, a cosine out of range) is zeros."""
    s = [np.ascontiguousarray(v, dtype=np.float32) for v in (sx, sy, sz)]
    q = [np.ascontiguousarray(v, dtype=np.float32) for v in (qx, qy, qz, ax, ay, az)]
    n = [None] * 3 if surface_normals is None else [np.ascontiguousarray(v, dtype=np.float32) for v in surface_normals]
    ns, nq, S = len(s[0]), len(q[0]), size(image_width)
    out = np.empty((nq, S), np.float32)
    raw = np.empty((nq, S), np.float64)
    sums = np.empty(nq, np.float64)
    stats = np.zeros(6, np.int64)
    p = lambda v: None if v is None else v.ctypes.data_as(_f32p)  # noqa: E731
    lib.spin_ref(*map(p, s), *map(p, n), ns, *map(p, q), nq, float(r), int(image_width), float(support_angle_cos),
                 int(min_pts_neighb), 1 if reversed_order else 0, out.ctypes.data_as(_f32p), raw.ctypes.data_as(_f64p),
                 sums.ctypes.data_as(_f64p), stats.ctypes.data_as(_i64p))
    return Result(out, raw, sums, *[int(v) for v in stats])


def eigen_sum(lib, m):
    m = np.ascontiguousarray(m, dtype=np.float64)
    return lib.spin_eigen_sum(m.ctypes.data_as(_f64p), len(m))


def eigen_sum_py(m):
    """Eigen 3.2's sum() of a double array, from Redux.h (packets of two doubles, two accumulators):
    four running sums over the indices = 0, 1, 2, 3 (mod 4) below 4 * (S // 4), combined lane-wise to
    (s0 + s2, s1 + s3), the next pair added lane-wise when S % 4 >= 2, the two lanes added, the last
    odd element added sequentially.  (One packet only, S < 4: m0 + m1, then the rest.)"""
    m = [np.float64(v) for v in m]
    S = len(m)
    if S == 0:
        return np.float64(0.0)
    if S < 4:
        res = m[0] + m[1] if S >= 2 else m[0]
        for v in m[2:]:
            res = res + v
        return res
    end2, end = 4 * (S // 4), 2 * (S // 2)
    s = m[:4]
    for i in range(4, end2):
        s[i % 4] = s[i % 4] + m[i]
    l0, l1 = s[0] + s[2], s[1] + s[3]
    if end > end2:
        l0, l1 = l0 + m[end2], l1 + m[end2 + 1]
    res = l0 + l1
    for v in m[end:]:
        res = res + v
    return res


def sequential_sum(m):
    res = np.float64(0.0)
    for v in m:
        res = res + np.float64(v)
    return res


def column_major(row, w):
    """A row in output index order (alpha_bin * (2w + 1) + beta_bin) -> Eigen's storage order."""
    return np.asarray(row).reshape(w + 1, 2 * w + 1).T.ravel()
