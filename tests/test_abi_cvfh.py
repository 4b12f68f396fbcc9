"""The CVFH and smooth-cluster entry points at the C-ABI.  Without a GPU: the symbols are declared in
include/pfx.h, exported by libpfx.so and bound, the header names what they replace and the five
statistics, the defaults are PCL's.  On the GPU: one case per PFX_ERR_INVALID of both forms (a null
required pointer, a negative size, a NaN or non-positive radius or tolerance, a NaN eps, min_points
below 1, an index out of range), each with its message from pfx_last_error, and the capacity rule of
the indexed count."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import cvfh_cases as K
from pcl_feature_extraction_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pfx_smooth_clusters", "pfx_smooth_clusters_dev", "pfx_cvfh", "pfx_cvfh_dev", "pfx_cvfh_params_default")
NAN = float("nan")


def test_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfx.h")).read(), flags=re.S)
    lib = N.lib()
    for name in SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m and hasattr(lib, name) and name in N.exported_symbols(), name
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
    assert set(SYMBOLS) <= N._OLDER_MAY_LACK   # an older library loaded for an A/B run lacks them
    names = lambda f: [a.split()[-1].lstrip("*") for a in re.search(r"\b" + f + r"\s*\(([^)]*)\)", text).group(1).split(",")]  # noqa: E731
    assert [a.replace("d_", "") for a in names("pfx_cvfh_dev")] == names("pfx_cvfh")
    assert [a.replace("d_", "") for a in names("pfx_smooth_clusters_dev")] == names("pfx_smooth_clusters")
    assert names("pfx_cvfh")[-7:] == ["params", "out", "cap", "n_rows", "centroids", "dominant_normals", "labels"]


def test_header_names_the_replaced_interface_and_the_statistics():
    text = open(os.path.join(ROOT, "include", "pfx.h")).read()
    head, body = text.split("#ifndef PFX_H_")[0], text.split("#ifndef PFX_H_")[1]
    assert "pfx_cvfh*" in head and "CVFHEstimation" in head and "649-675" in head and "pfx_smooth_clusters*" in head
    for stat in ("cvfh_filtered", "cvfh_clusters", "cvfh_edges", "cvfh_cc_rounds", "cvfh_rows"):
        assert '"' + stat + '"' in body, stat
    assert re.search(r"#define\s+PFX_CVFH_DIM\s+308\b", body)


def test_defaults_are_pcl_s():
    from pcl_feature_extraction_amd import cvfh_params
    f, p = np.float32, cvfh_params()
    assert ctypes.sizeof(N.CvfhParams) == 36
    assert list(p.viewpoint) == [0, 0, 0] and p.radius_normals == f(0.005) * f(3) == p.cluster_tolerance
    assert p.eps_angle_threshold == f(0.125) and p.curvature_threshold == f(0.03)
    assert (p.min_points, p.normalize_bins) == (50, 0)


def test_python_signatures():
    from pcl_feature_extraction_amd import Context
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(Context.smooth_clusters) == ["self", "x", "y", "z", "nx", "ny", "nz", "tolerance", "eps_angle",
                                               "min_points"]
    assert params(Context.smooth_clusters_dev) == params(Context.smooth_clusters) + ["labels", "n_clusters"]
    assert params(Context.cvfh) == ["self", "sx", "sy", "sz", "snx", "sny", "snz", "scurvature", "indices", "params",
                                    "cap"]
    assert params(Context.cvfh_dev)[:11] == ["self", "sx", "sy", "sz", "snx", "sny", "snz", "scurvature", "indices",
                                             "out", "n_rows"]


# ---- on the GPU ----

def raw(v):
    """An array or tensor as the pointer the C-ABI takes; every other argument as it is."""
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v


def both_forms(host):
    import torch
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    dev = [up(v) if isinstance(v, np.ndarray) else v for v in host]
    torch.cuda.synchronize()
    return {"": host, "_dev": dev}


def refused(ctx, fn, args, code, words):
    assert fn(ctx.h, *[raw(v) for v in args]) == code, words
    msg = ctx._lib.pfx_last_error(ctx.h).decode()
    assert words in msg, msg


@pytest.mark.gpu
def test_smooth_clusters_argument_rule(ctx):
    xyz, _ = K.islands((60,))
    nrm = K.flat_normals(60)[:3]
    host = [*xyz, *nrm, 60, float(K.TOL), 0.125, 50, np.full(60, 7, np.int32), np.zeros(1, np.int64)]
    for form, args in both_forms(host).items():
        fn = getattr(ctx._lib, "pfx_smooth_clusters" + form)
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK, ctx._lib.pfx_last_error(ctx.h)
        ctx.synchronize()
        for i in (0, 1, 2, 3, 4, 5, 10, 11):
            refused(ctx, fn, args[:i] + [None] + args[i + 1:], N.PFX_ERR_INVALID, "smooth_clusters: invalid arguments")
        edit = lambda i, v: args[:i] + [v] + args[i + 1:]  # noqa: E731
        refused(ctx, fn, edit(6, -1), N.PFX_ERR_INVALID, "invalid arguments")
        for t in (0.0, -0.01, NAN):
            refused(ctx, fn, edit(7, t), N.PFX_ERR_INVALID, "the tolerance must be > 0")
        refused(ctx, fn, edit(8, NAN), N.PFX_ERR_INVALID, "eps_angle is NaN")
        refused(ctx, fn, edit(9, 0), N.PFX_ERR_INVALID, "min_points must be >= 1")
        assert ctx._lib.pfx_smooth_clusters(None, *[raw(v) for v in host]) == N.PFX_ERR_INVALID
        # n == 0 needs no pointer and gives no cluster
        assert fn(ctx.h, None, None, None, None, None, None, 0, float(K.TOL), 0.125, 50, None, raw(args[11])) == N.PFX_OK
        ctx.synchronize()
    assert host[11][0] == 0
    # an eps beyond pi joins whatever is near; a negative one nothing
    labels, n = ctx.smooth_clusters(*xyz, *nrm, K.TOL, 4.0, 50)
    assert n == 1 and set(labels) == {0}
    labels, n = ctx.smooth_clusters(*xyz, *nrm, K.TOL, -1.0, 1)
    assert n == 60 and labels.tolist() == list(range(60))


@pytest.mark.gpu
def test_cvfh_argument_rule(ctx):
    from pcl_feature_extraction_amd import cvfh_params
    xyz, _ = K.islands((60,))
    s = list(xyz + K.flat_normals(60))
    idx = np.arange(60, dtype=np.int32)

    def call(p, indices=idx, n_idx=60, ns=60):
        return [*s, ns, indices, n_idx, ctypes.byref(p), np.zeros((2, 308), np.float32), 2, np.zeros(1, np.int64),
                np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), np.zeros(60, np.int32)]

    for form in ("", "_dev"):
        fn = getattr(ctx._lib, "pfx_cvfh" + form)
        args = call(cvfh_params())
        if form:
            args = both_forms(args)["_dev"]
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK, ctx._lib.pfx_last_error(ctx.h)
        ctx.synchronize()
        edit = lambda i, v: args[:i] + [v] + args[i + 1:]  # noqa: E731
        for i in (0, 1, 2, 3, 4, 5, 6, 10, 11, 13):     # the required pointers (11: out with cap > 0)
            refused(ctx, fn, edit(i, None), N.PFX_ERR_INVALID, "cvfh: invalid arguments")
        for i in (14, 15, 16):                          # the optional outputs
            assert fn(ctx.h, *[raw(v) for v in edit(i, None)]) == N.PFX_OK
            ctx.synchronize()
        refused(ctx, fn, edit(7, -1), N.PFX_ERR_INVALID, "invalid arguments")
        refused(ctx, fn, edit(9, -1), N.PFX_ERR_INVALID, "invalid arguments")
        refused(ctx, fn, edit(12, -1), N.PFX_ERR_INVALID, "invalid arguments")
        refused(ctx, fn, edit(8, None)[:9] + [59] + args[10:], N.PFX_ERR_INVALID, "invalid arguments")  # all, but 59
        for field, bad, words in (("radius_normals", (0.0, -1.0, NAN), "radius_normals must be > 0"),
                                  ("cluster_tolerance", (0.0, -1.0, NAN), "cluster_tolerance must be > 0"),
                                  ("eps_angle_threshold", (NAN,), "eps_angle_threshold is NaN"),
                                  ("min_points", (0, -3), "min_points must be >= 1")):
            for v in bad:
                p = cvfh_params()
                setattr(p, field, v)
                refused(ctx, fn, edit(10, ctypes.byref(p)), N.PFX_ERR_INVALID, words)
        for where, v in ((0, -1), (59, 60), (30, 1 << 30)):
            bad = idx.copy()
            bad[where] = v
            b = edit(8, both_forms([bad])["_dev"][0] if form else bad)
            refused(ctx, fn, b, N.PFX_ERR_INVALID, "an index is outside the surface")
        refused(ctx, fn, edit(9, (1 << 24) + 1), N.PFX_ERR_CAPACITY, "2^24")
        # the context is usable afterwards
        assert fn(ctx.h, *[raw(v) for v in args]) == N.PFX_OK
        ctx.synchronize()
    assert ctx._lib.pfx_cvfh(None, *[raw(v) for v in call(cvfh_params())]) == N.PFX_ERR_INVALID
