"""Thin ctypes wrapper around tests/cpp/knn_ref.cpp, the CPU restatement of DESIGN.md "k-NN: the
contract" (test infrastructure: nothing under pcl_feature_extraction_amd/ uses it)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "knn_ref.cpp")

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


def build(out_dir):
    """Compile knn_ref.cpp into out_dir (the oracle's flags: -O2, no FMA contraction, plain x86-64,
    OpenMP over the queries) and load it."""
    so = os.path.join(str(out_dir), "libknn_ref.so")
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-shared", "-fPIC",
           "-I", os.path.join(ROOT, "oracle"), SRC, "-o", so]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(so)
    lib.knn_ref_search.restype = ctypes.c_int
    lib.knn_ref_search.argtypes = [_f32p] * 3 + [ctypes.c_int64] + [_f32p] * 3 + [ctypes.c_int64, ctypes.c_int32,
                                                                                  _i64p, _i32p, _f32p, _i64p]
    lib.knn_ref_normals.restype = ctypes.c_int
    lib.knn_ref_normals.argtypes = [_f32p] * 3 + [ctypes.c_int64, ctypes.c_int32] + [ctypes.c_float] * 3 + [_f32p] * 4
    return lib


def _f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


def search(lib, x, y, z, qx, qy, qz, k, ties=False):
    """(counts (nq,) int64, idx (nq, k) int32, d2 (nq, k) float32); with ties also (queries with an
    equal d2 inside the row, queries whose k-th d2 equals the next one's)."""
    x, y, z, qx, qy, qz = map(_f32, (x, y, z, qx, qy, qz))
    nq = len(qx)
    counts = np.zeros(nq, np.int64)
    idx = np.zeros((nq, k), np.int32)
    d2 = np.zeros((nq, k), np.float32)
    t = np.zeros(2, np.int64)
    st = lib.knn_ref_search(*(v.ctypes.data_as(_f32p) for v in (x, y, z)), len(x),
                            *(v.ctypes.data_as(_f32p) for v in (qx, qy, qz)), nq, k, counts.ctypes.data_as(_i64p),
                            idx.ctypes.data_as(_i32p), d2.ctypes.data_as(_f32p), t.ctypes.data_as(_i64p))
    assert st == 0
    return (counts, idx, d2, (int(t[0]), int(t[1]))) if ties else (counts, idx, d2)


def prefix(rows, k):
    """The rows of a search at a smaller k from those at a larger one: the first k of each row (the
    contract orders a row by one key, so the smaller search is its prefix)."""
    counts, idx, d2 = rows[:3]
    return np.minimum(counts, k), np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k])


def normals(lib, x, y, z, k, viewpoint=(0.0, 0.0, 0.0)):
    x, y, z = map(_f32, (x, y, z))
    n = len(x)
    out = np.zeros((4, n), np.float32)
    st = lib.knn_ref_normals(*(v.ctypes.data_as(_f32p) for v in (x, y, z)), n, k, *(float(np.float32(v)) for v in viewpoint),
                             *(out[i].ctypes.data_as(_f32p) for i in range(4)))
    assert st == 0
    return out[0], out[1], out[2], out[3]
