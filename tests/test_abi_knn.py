"""The k-NN entry points at the C-ABI.  Without a GPU: the symbols are declared in include/pfx.h,
exported by libpfx.so and bound with as many arguments as declared, the _dev forms take the host
forms' arguments, the header names what they replace, the tie rule and the statistics, and
KNN_MAX_K is the header's PFX_KNN_MAX_K.  On the GPU: one case per PFX_ERR_INVALID of all four forms
(a null required pointer, a negative size, k below 1), each with its message, k beyond the maximum as
PFX_ERR_CAPACITY, and the calls that need no pointer."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import knn_cases as C
from pcl_feature_extraction_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pfx_knn_search", "pfx_knn_search_dev", "pfx_normals_knn", "pfx_normals_knn_dev")


def test_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfx.h")).read(), flags=re.S)
    lib = N.lib()
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m and hasattr(lib, name) and name in N.exported_symbols(), name
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
    assert set(SYMBOLS) <= N._OLDER_MAY_LACK   # an older library loaded for an A/B run lacks them
    names = lambda f: [re.sub(r"\[\d*\]", "", a.split()[-1].lstrip("*")) for a in  # noqa: E731
                       re.search(r"\b" + f + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    assert [re.sub(r"^d_", "", a) for a in names("pfx_knn_search_dev")] == names("pfx_knn_search")
    assert [re.sub(r"^d_", "", a) for a in names("pfx_normals_knn_dev")] == names("pfx_normals_knn")
    assert names("pfx_knn_search")[-4:] == ["k", "counts", "idx", "d2"]
    assert names("pfx_normals_knn")[4:7] == ["n", "k", "viewpoint"]


def test_header_names_the_contract_and_the_statistics():
    text = open(os.path.join(ROOT, "include", "pfx.h")).read()
    head, body = text.split("#ifndef PFX_H_")[0], text.split("#ifndef PFX_H_")[1]
    assert "pfx_knn_search*" in head and "nearestKSearch" in head and "pfx_normals_knn*" in head and "setKSearch" in head
    for stat in ("knn_queries", "knn_rounds", "knn_first", "knn_requeued", "knn_exhaustive", "knn_skipped"):
        assert '"' + stat + '"' in body, stat
    assert 'DESIGN.md "k-NN: the contract"' in body and "ties are broken by index" in body
    m = re.search(r"#define\s+PFX_KNN_MAX_K\s+(\d+)\b", body)
    assert m and int(m.group(1)) == N.KNN_MAX_K >= 256


def test_python_signatures():
    from pcl_feature_extraction_amd import Context
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(Context.knn_search) == ["self", "x", "y", "z", "qx", "qy", "qz", "k"]
    assert params(Context.knn_search_dev) == params(Context.knn_search) + ["counts", "idx", "d2"]
    assert params(Context.normals_knn) == ["self", "x", "y", "z", "k", "viewpoint"]
    assert params(Context.normals_knn_dev) == ["self", "x", "y", "z", "k", "nx", "ny", "nz", "curv", "viewpoint"]
    assert inspect.signature(Context.normals_knn).parameters["viewpoint"].default == (0.0, 0.0, 0.0)


# ---- on the GPU ----

def raw(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v


def forms(host):
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v for v in host]
    torch.cuda.synchronize()
    return {"": host, "_dev": dev}


def refused(ctx, fn, args, code, words):
    assert fn(ctx.h, *[raw(v) for v in args]) == code, words
    msg = ctx._lib.pfx_last_error(ctx.h).decode()
    assert words in msg, msg


@pytest.mark.gpu
def test_knn_search_argument_rule(ctx):
    s, q = C.short(), C.single()
    host = [*s, 5, *q, 1, 3, np.zeros(1, np.int64), np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32)]
    for form, args in forms(host).items():
        fn = getattr(ctx._lib, "pfx_knn_search" + form)
        edit = lambda i, v: args[:i] + [v] + args[i + 1:]  # noqa: E731
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK, ctx._lib.pfx_last_error(ctx.h)
        ctx.synchronize()
        for i in (0, 1, 2, 4, 5, 6, 9, 10, 11):
            refused(ctx, fn, edit(i, None), N.PFX_ERR_INVALID, "knn_search: invalid arguments")
        refused(ctx, fn, edit(3, -1), N.PFX_ERR_INVALID, "knn_search: invalid arguments")
        refused(ctx, fn, edit(7, -1), N.PFX_ERR_INVALID, "knn_search: invalid arguments")
        refused(ctx, fn, edit(3, 1 << 28), N.PFX_ERR_CAPACITY, "2^28")
        refused(ctx, fn, edit(7, 1 << 28), N.PFX_ERR_CAPACITY, "2^28")
        for k in (0, -1):
            refused(ctx, fn, edit(8, k), N.PFX_ERR_INVALID, "k must be >= 1")
        refused(ctx, fn, edit(8, N.KNN_MAX_K + 1), N.PFX_ERR_CAPACITY, "PFX_KNN_MAX_K")
        # no surface needs no surface pointer, no query no query pointer or output
        assert fn(ctx.h, None, None, None, 0, *[raw(v) for v in args[4:]]) == N.PFX_OK
        assert fn(ctx.h, *[raw(v) for v in args[:4]], None, None, None, 0, 3, None, None, None) == N.PFX_OK
        ctx.synchronize()
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK   # the context is usable afterwards
        ctx.synchronize()
    assert ctx._lib.pfx_knn_search(None, *[raw(v) for v in host]) == N.PFX_ERR_INVALID
    assert host[9][0] == 3 and sorted(set(host[10][0].tolist())) == sorted(host[10][0].tolist())
    assert ((host[10][0] >= 0) & (host[10][0] < 5)).all() and (np.diff(host[11][0]) >= 0).all()


@pytest.mark.gpu
def test_normals_knn_argument_rule(ctx):
    s = C.short()
    vp = np.zeros(3, np.float32)
    host = [*s, 5, 3, vp, *(np.zeros(5, np.float32) for _ in range(4))]
    for form, args in forms(host).items():
        args[5] = vp     # the viewpoint is read on the host in both forms
        fn = getattr(ctx._lib, "pfx_normals_knn" + form)
        edit = lambda i, v: args[:i] + [v] + args[i + 1:]  # noqa: E731
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK, ctx._lib.pfx_last_error(ctx.h)
        ctx.synchronize()
        for i in (0, 1, 2, 6, 7, 8, 9):
            refused(ctx, fn, edit(i, None), N.PFX_ERR_INVALID, "normals_knn: invalid arguments")
        assert fn(ctx.h, *[raw(v) for v in edit(5, None)]) == N.PFX_OK     # viewpoint NULL: the origin
        ctx.synchronize()
        refused(ctx, fn, edit(3, -1), N.PFX_ERR_INVALID, "normals_knn: invalid arguments")
        refused(ctx, fn, edit(4, 0), N.PFX_ERR_INVALID, "k must be >= 1")
        refused(ctx, fn, edit(4, N.KNN_MAX_K + 1), N.PFX_ERR_CAPACITY, "PFX_KNN_MAX_K")
        refused(ctx, fn, edit(3, 1 << 28), N.PFX_ERR_CAPACITY, "2^28")
        assert fn(ctx.h, None, None, None, 0, 3, None, None, None, None, None) == N.PFX_OK
        ctx.synchronize()
    assert np.isfinite(host[6]).all()
