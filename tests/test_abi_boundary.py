"""The boundary-point entry points at the C-ABI.  Without a GPU: the symbols are declared in
include/pfx.h, exported by libpfx.so and bound with the header's argument lists, and the Python
front-end has the signatures and the constant the issue states.  On the GPU: the argument rule of
both forms (a null required pointer, a negative size, a null context, a bad radius, a NaN threshold
are PFX_ERR_INVALID before anything is copied or launched), a threshold below pi / 64 is
PFX_ERR_UNSUPPORTED, nq == 0 is a no-op and n_surface == 0 fills the rows with 255."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import boundary_cases as K
from pcl_feature_extraction_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pfx_boundary", "pfx_boundary_dev")
PI_64 = float(np.float32(math.pi / 64))


def _prototypes():
    src = open(os.path.join(ROOT, "include", "pfx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"pfx_status\s+(pfx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_symbols_declared_exported_and_bound():
    protos, lib = _prototypes(), N.lib()
    kinds = {"pfx_ctx*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p,
             "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}
    for name in SYMBOLS:
        assert name in protos and hasattr(lib, name) and name in N.exported_symbols(), name
        want = [kinds[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in protos[name]]
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 or fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want, name
    names = lambda f: [a.split()[-1].lstrip("*") for a in protos[f]]  # noqa: E731
    assert names("pfx_boundary") == ["ctx", "sx", "sy", "sz", "n_surface", "qx", "qy", "qz", "qnx", "qny", "qnz", "nq",
                                     "radius", "angle_threshold", "out"]
    assert [a.replace("d_", "") for a in names("pfx_boundary_dev")] == names("pfx_boundary")
    assert set(SYMBOLS) <= N._OLDER_MAY_LACK   # an older library loaded for an A/B run lacks them


def test_header_names_the_replaced_interface_and_the_constant():
    import pcl_feature_extraction_amd as pkg
    text = open(os.path.join(ROOT, "include", "pfx.h")).read()
    head = text.split("#ifndef PFX_H_")[0]
    assert "pfx_boundary*" in head and "BoundaryEstimation" in head and "394-415" in head
    body = text.split("#ifndef PFX_H_")[1]
    for stat in ("boundary_neighbors", "boundary_kmax", "boundary_flagged"):
        assert '"' + stat + '"' in body, stat
    assert re.search(r"#define\s+PFX_BOUNDARY_NO_NEIGHBORS\s+255\b", body)
    assert pkg.BOUNDARY_NO_NEIGHBORS == 255 and "BOUNDARY_NO_NEIGHBORS" in pkg.__all__


def test_python_signatures():
    from pcl_feature_extraction_amd import Context
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(Context.boundary) == ["self", "sx", "sy", "sz", "qx", "qy", "qz", "qnx", "qny", "qnz", "r",
                                        "angle_threshold"]
    assert params(Context.boundary_dev) == ["self", "sx", "sy", "sz", "qx", "qy", "qz", "qnx", "qny", "qnz", "r", "out",
                                            "angle_threshold"]
    for f in (Context.boundary, Context.boundary_dev):
        assert inspect.signature(f).parameters["angle_threshold"].default == math.pi / 2


# ---- on the GPU ----

def raw(v):
    """An array or tensor as the pointer the C-ABI takes; every other argument as it is."""
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v


@pytest.fixture(scope="module")
def forms():
    """The arguments after ctx of a valid call of either form on the 9 x 9 lattice, every point a
    query: {"": host arrays, "_dev": device tensors}."""
    import torch
    xyz, nrm, _ = K.lattice()
    dev = torch.device("cuda", 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    host = [*xyz, 81, *xyz, *nrm, 81, 0.025, math.pi / 2, np.full(81, 7, np.uint8)]
    device = [up(v) if isinstance(v, np.ndarray) else v for v in host]
    torch.cuda.synchronize()
    return {"": host, "_dev": device}


REQUIRED = [0, 1, 2, 4, 5, 6, 7, 8, 9, 13]   # the pointers; 3 and 10 are n_surface and nq, 11 the radius, 12 the threshold


@pytest.mark.gpu
def test_argument_rule_of_both_forms(ctx, forms):
    import torch
    lib = ctx._lib
    rim = K.lattice()[2].astype(np.uint8)
    for form, args in forms.items():
        fn, what = getattr(lib, "pfx_boundary" + form), "pfx_boundary" + form
        a = [raw(v) for v in args]
        assert fn(ctx.h, *a) == N.PFX_OK, (what, lib.pfx_last_error(ctx.h))
        ctx.synchronize()
        for i in REQUIRED:
            b = list(a)
            b[i] = None
            assert fn(ctx.h, *b) == N.PFX_ERR_INVALID, (what, "null argument", i)
            assert lib.pfx_last_error(ctx.h).decode() == "boundary: invalid arguments", (what, i)
        for i in (3, 10):
            b = list(a)
            b[i] = -1
            assert fn(ctx.h, *b) == N.PFX_ERR_INVALID, (what, "negative size", i)
        assert fn(None, *a) == N.PFX_ERR_INVALID, (what, "null ctx")
        for r in (0.0, -1.0, float("nan")):
            b = list(a)
            b[11] = r
            assert fn(ctx.h, *b) == N.PFX_ERR_INVALID, (what, "radius", r)
        b = list(a)
        b[12] = float("nan")
        assert fn(ctx.h, *b) == N.PFX_ERR_INVALID, (what, "NaN threshold")
        # below pi / 64 (as a float32): unsupported, with the reason; at it and above: served
        for t in (float(np.nextafter(np.float32(PI_64), np.float32(0))), 0.0, -1.0, float("-inf")):
            b[12] = t
            assert fn(ctx.h, *b) == N.PFX_ERR_UNSUPPORTED, (what, t)
            assert "pi / 64" in lib.pfx_last_error(ctx.h).decode() and "bin" in lib.pfx_last_error(ctx.h).decode()
        for t in (PI_64, 7.0, float("inf")):
            b[12] = t
            assert fn(ctx.h, *b) == N.PFX_OK, (what, t)
            ctx.synchronize()
    # nothing of the rejected calls was copied or run: both forms hold the lattice's flags at the last
    # served threshold (infinite: no boundary), then at pi / 2 its rim
    torch.cuda.synchronize()
    assert not forms[""][-1].any() and not forms["_dev"][-1].cpu().numpy().any()
    for form, args in forms.items():
        assert getattr(lib, "pfx_boundary" + form)(ctx.h, *[raw(v) for v in args]) == N.PFX_OK
        ctx.synchronize()
    assert np.array_equal(forms[""][-1], rim) and np.array_equal(forms["_dev"][-1].cpu().numpy(), rim)
    assert (ctx.stat("boundary_kmax"), ctx.stat("boundary_flagged")) == (21, 32)


@pytest.mark.gpu
def test_no_queries_is_a_no_op_and_no_surface_fills_255(ctx, forms):
    import torch
    lib = ctx._lib
    assert lib.pfx_boundary(ctx.h, *[raw(v) for v in forms[""]]) == N.PFX_OK
    kmax = ctx.stat("boundary_kmax")
    assert kmax == 21
    for form, args in forms.items():
        fn = getattr(lib, "pfx_boundary" + form)
        # nq == 0: null query and output pointers and all; nothing is written, run or reported
        out = args[-1]
        if form:
            out.fill_(9)
            torch.cuda.synchronize()
        else:
            out.fill(9)
        b = [raw(v) for v in args]
        b[4:11] = [None] * 6 + [0]
        b[13] = None
        assert fn(ctx.h, *b) == N.PFX_OK, form
        ctx.synchronize()
        assert ctx.stat("boundary_kmax") == kmax
        got = out.cpu().numpy() if form else out
        assert (got == 9).all()
        # n_surface == 0: null surface pointers and all; every row is PFX_BOUNDARY_NO_NEIGHBORS
        b = [raw(v) for v in args]
        b[0:4] = [None] * 3 + [0]
        assert fn(ctx.h, *b) == N.PFX_OK, form
        ctx.synchronize()
        got = out.cpu().numpy() if form else out
        assert (got == 255).all(), form
        assert (ctx.stat("boundary_neighbors"), ctx.stat("boundary_kmax"), ctx.stat("boundary_flagged")) == (0, 0, 0)
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK   # (the statistics of a real call again)
        ctx.synchronize()
