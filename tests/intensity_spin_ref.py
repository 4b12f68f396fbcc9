"""Thin ctypes wrapper around tests/cpp/intensity_spin_ref.cpp, the CPU restatement of PCL 1.7
IntensitySpinEstimation with the exponential of csrc/pfx_expf.h (test infrastructure: nothing under
pcl_feature_extraction_amd/ uses it)."""
import collections
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "intensity_spin_ref.cpp")

_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)

#: out (nq, D I) float32, then the counts
Result = collections.namedtuple("Result", "out neighbors kmax")


def build(out_dir):
    """Compile intensity_spin_ref.cpp into out_dir (the oracle's floating-point contract: -O2, no FMA
    contraction, plain x86-64) and load it."""
    so = os.path.join(str(out_dir), "libintensity_spin_ref.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wl,-z,defs", "-I",
           os.path.join(ROOT, "oracle"), SRC, "-o", so]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(so)
    lib.ispin_ref.restype = None
    lib.ispin_ref.argtypes = ([_f32p] * 4 + [ctypes.c_int64] + [_f32p] * 3 +
                              [ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                               ctypes.c_int, _f32p, _i64p])
    for f in (lib.ispin_expf, lib.ispin_libm_expf):
        f.restype = ctypes.c_float
        f.argtypes = [ctypes.c_float]
    lib.ispin_expf_compare.restype = ctypes.c_float
    lib.ispin_expf_compare.argtypes = [_f32p, ctypes.c_int64, _i64p, _i64p]
    return lib


def _arrs(*a):
    return [np.ascontiguousarray(v, dtype=np.float32) for v in a]


def _p(v):
    return v.ctypes.data_as(_f32p)


def spin(lib, sx, sy, sz, si, cx, cy, cz, r, nr_distance_bins=4, nr_intensity_bins=5, sigma=1.0,
         reversed_order=False):
    """The intensity spin images' rows, (nq, D I): row[dj * I + ii]."""
    a = _arrs(sx, sy, sz, si, cx, cy, cz)
    ns, nq = len(a[0]), len(a[4])
    out = np.empty((nq, nr_distance_bins * nr_intensity_bins), np.float32)
    stats = np.zeros(2, np.int64)
    lib.ispin_ref(*map(_p, a[:4]), ns, *map(_p, a[4:]), nq, float(r), int(nr_distance_bins), int(nr_intensity_bins),
                  float(sigma), 1 if reversed_order else 0, _p(out), stats.ctypes.data_as(_i64p))
    return Result(out, int(stats[0]), int(stats[1]))


def expf(lib, x):
    """pfx_expf of one float, as a numpy float32."""
    return np.float32(lib.ispin_expf(ctypes.c_float(float(x))))


def libm_expf(lib, x):
    return np.float32(lib.ispin_libm_expf(ctypes.c_float(float(x))))


def expf_compare(lib, x):
    """pfx_expf against the host libm's expf over the float32 array x: (the counts of arguments 0, 1
    and more ulps apart, the count of NaN / zero / infinity disagreements, the first argument more than
    one ulp apart or 0)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hist = np.zeros(3, np.int64)
    mismatch = np.zeros(1, np.int64)
    worst = lib.ispin_expf_compare(_p(x), len(x), hist.ctypes.data_as(_i64p), mismatch.ctypes.data_as(_i64p))
    return hist, int(mismatch[0]), float(worst)
