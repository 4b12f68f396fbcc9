"""The argument rule of the 26 descriptor entry points (13 families, a host and a device form each),
straight at the C-ABI: a valid call passes; a null required pointer, a negative size and a null
context are PFX_ERR_INVALID before anything is copied or launched; the host forms then give the
same bits as before.

The table below is read off csrc/pfx_api.hip (each family's *_rule).  It leaves the optional
arguments alone -- the spin image's surface normals without a support angle and its raw / sums, the
shape context's rnd, FPFH's queries under same_as_surface (every call here passes same_as_surface
= 0, where they are required) -- because a null pointer the rule lets through would reach a kernel
in the device forms.
"""
import ctypes

import numpy as np
import pytest

import rift_cases as K
from parity import bits

pytestmark = pytest.mark.gpu

N = 8                               # points of the cloud, all of them queries
R, RMIN, RHO = 0.05, 0.005, 0.01    # the search radius; the shape contexts' minimal and density radii


def table(a, new, prm):
    """family -> (arguments after ctx, positions of the required pointers, positions of n_surface and
    nq, outputs).  a: the input arrays, new(width): a fresh (N, width) float32 output."""
    s, n, g, si, rgb, fr = a["s"], a["n"], a["g"], a["i"], a["rgb"], a["frames"]
    q, qn = s, n                    # the queries are the surface points, with their normals
    t = {}

    def add(name, args, required, sizes):  # (the outputs are the arrays that follow nq)
        t[name] = (args, required, sizes, [v for v in args[sizes[1]:] if hasattr(v, "shape")])

    add("fpfh", [*s, *n, N, *q, N, 0, R, new(33)], [0, 1, 2, 3, 4, 5, 7, 8, 9, 13], (6, 10))
    add("shot", [*s, *n, N, *q, N, R, new(352), new(9)], [0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13], (6, 10))
    add("shot_color", [*s, *n, rgb, N, *q, rgb, N, R, new(1344), new(9)],
        [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 14, 15], (7, 12))
    add("pfh", [*s, *n, N, *q, N, R, new(125)], [0, 1, 2, 3, 4, 5, 7, 8, 9, 12], (6, 10))
    add("spin_image", [*s, *n, N, *q, *qn, N, R, prm, new(153), None, None],
        [0, 1, 2, 7, 8, 9, 10, 11, 12, 15, 16], (6, 13))
    add("intensity_gradient", [*s, si, N, *q, *qn, N, 0, R, new(3)], [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 14], (4, 11))
    add("rift", [*s, *g, N, *q, N, R, 4, 4, new(16)], [0, 1, 2, 3, 4, 5, 7, 8, 9, 14], (6, 10))
    add("intensity_spin", [*s, si, N, *q, N, R, 4, 5, 1.0, new(20)], [0, 1, 2, 3, 5, 6, 7, 13], (4, 8))
    add("moment_invariants", [*s, N, *q, N, R, new(3)], [0, 1, 2, 4, 5, 6, 9], (3, 7))
    add("principal_curvatures", [*s, *n, N, *q, *qn, N, R, new(5)],
        [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 15], (6, 13))
    add("shape_context", [*s, *n, N, *q, N, R, RMIN, RHO, None, new(1980), new(9)],
        [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16], (6, 10))
    add("usc", [*s, N, *q, fr, N, R, RMIN, RHO, new(1980), new(9)], [0, 1, 2, 4, 5, 6, 7, 12, 13], (3, 8))
    add("shot_lrf", [*s, N, *q, N, R, new(9)], [0, 1, 2, 4, 5, 6, 9], (3, 7))
    return t


def raw(v):
    """An array or tensor as the pointer the C-ABI takes; every other argument as it is."""
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v


def test_descriptor_argument_rules():
    import torch
    from pcl_feature_extraction_amd import Context
    from pcl_feature_extraction_amd._native import PFX_ERR_INVALID, SpinParams
    c = K.order_case(k=N, blobs=1)
    frames = np.tile(np.eye(3, dtype=np.float32).ravel(), (N, 1))
    host = dict(s=c["xyz"], n=c["normals"], g=c["gradients"], i=c["intensity"], frames=frames,
                rgb=np.random.default_rng(7).integers(0, 1 << 24, N, dtype=np.uint32))
    assert all(len(v) == N for v in (*host["s"], *host["n"], *host["g"], host["i"]))
    dev = torch.device("cuda", 0)

    def up(v):
        if isinstance(v, tuple):
            return tuple(up(w) for w in v)
        return torch.from_numpy(np.ascontiguousarray(v).view(np.int32 if v.dtype == np.uint32 else v.dtype)).to(dev)

    with Context(0) as ctx:
        lib = ctx._lib
        prm = SpinParams()
        lib.pfx_spin_params_default(ctypes.byref(prm))
        prm = ctypes.pointer(prm)
        forms = {"": table(host, lambda w: np.full((N, w), -1.0, np.float32), prm),
                 "_dev": table({k: up(v) for k, v in host.items()},
                               lambda w: torch.full((N, w), -1.0, dtype=torch.float32, device=dev), prm)}
        torch.cuda.synchronize()
        before = {}
        for form, t in forms.items():
            assert len(t) == 13
            for name, (args, required, sizes, outs) in t.items():
                fn, what = getattr(lib, f"pfx_{name}{form}"), f"pfx_{name}{form}"
                a = [raw(v) for v in args]
                assert fn(ctx.h, *a) == 0, (what, lib.pfx_last_error(ctx.h))
                if not form:
                    before[name] = [o.copy() for o in outs]
                for i in required:
                    assert a[i] is not None and not isinstance(a[i], (int, float)), (what, i)
                    b = list(a)
                    b[i] = None
                    assert fn(ctx.h, *b) == PFX_ERR_INVALID, (what, "null argument", i)
                    msg = lib.pfx_last_error(ctx.h).decode()
                    assert msg == f"{name}: invalid arguments", (what, i, msg)
                for i in sizes:
                    assert a[i] == N
                    b = list(a)
                    b[i] = -1
                    assert fn(ctx.h, *b) == PFX_ERR_INVALID, (what, "negative size", i)
                assert fn(None, *a) == PFX_ERR_INVALID, (what, "null ctx")
        ctx.synchronize()
        # the texts keep their family's name in front (checked for every rejection above; the three
        # the issue names, once more by hand)
        for name, null in (("fpfh", 0), ("shot", 3), ("shape_context", 15)):
            a = [raw(v) for v in forms[""][name][0]]
            a[null] = None
            assert getattr(lib, f"pfx_{name}")(ctx.h, *a) == PFX_ERR_INVALID
            assert lib.pfx_last_error(ctx.h).decode().startswith(name + ":")
        # nothing of the rejected calls was copied or run: every host form computes what it did
        for name, (args, _, _, outs) in forms[""].items():
            for o in outs:
                o.fill(-1.0)
            assert getattr(lib, f"pfx_{name}")(ctx.h, *[raw(v) for v in args]) == 0, name
            assert len(outs) == len(before[name]) >= 1
            for o, want in zip(outs, before[name]):
                assert np.array_equal(bits(o), bits(want)), name
        # and the valid calls computed something: a point of this blob has all eight as neighbours
        assert np.isfinite(before["fpfh"][0]).all() and np.isfinite(before["moment_invariants"][0]).all()
