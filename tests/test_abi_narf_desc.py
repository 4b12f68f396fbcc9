"""The NARF descriptor and point-index entry points at the C-ABI.  Without a GPU: the symbols are
declared in include/pfx.h, exported by libpfx.so and bound with the header's argument lists, the
defaults are the issue's, and the Python front-end has its signatures.  On the GPU: the argument rule of
both forms (a null required pointer, a negative size, a null context, support_size <= 0 or NaN are
PFX_ERR_INVALID before anything is copied or launched), the camera's bounds, the capacity behaviour
with cap one below and at the row count, nk == 0 and n == 0."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import narf_desc_cases as K
from pcl_feature_extraction_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pfx_narf_descriptors", "pfx_narf_descriptors_dev", "pfx_point_indices", "pfx_point_indices_dev")


def _prototypes():
    src = open(os.path.join(ROOT, "include", "pfx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"pfx_status\s+(pfx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_symbols_declared_exported_and_bound():
    protos, lib = _prototypes(), N.lib()
    vp = ctypes.c_void_p
    kinds = {"pfx_ctx*": vp, "const float*": vp, "float*": vp, "const int32_t*": vp, "int32_t*": vp, "int64_t": ctypes.c_int64,
             "float": ctypes.c_float, "const pfx_camera*": ctypes.POINTER(N.Camera),
             "const pfx_narf_desc_params*": ctypes.POINTER(N.NarfDescParams)}
    for name in SYMBOLS:
        assert name in protos and hasattr(lib, name) and name in N.exported_symbols(), name
        args = protos[name]
        want = [kinds[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in args[:-1]]
        # the count: a host int64_t* in the host form, a device pointer in the _dev form
        assert re.sub(r"\s*\w+$", "", args[-1]) == "int64_t*"
        want.append(vp if name.endswith("_dev") else N.c_i64p)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 or fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want, name
    names = lambda f: [a.split()[-1].lstrip("*") for a in protos[f]]  # noqa: E731
    assert names("pfx_narf_descriptors") == ["ctx", "x", "y", "z", "n", "cam", "pixel_idx", "nk", "params", "desc", "pose",
                                             "row_key", "cap", "n_out"]
    assert names("pfx_point_indices") == ["ctx", "x", "y", "z", "n", "kx", "ky", "kz", "nk", "tol", "out", "cap", "n_out"]
    for f in ("pfx_narf_descriptors", "pfx_point_indices"):
        assert [a.replace("d_", "") for a in names(f + "_dev")] == names(f)
    assert set(SYMBOLS) | {"pfx_narf_desc_params_default"} <= N._OLDER_MAY_LACK


def test_defaults_and_header():
    p = N.NarfDescParams()
    p.support_size, p.rotation_invariant = 7.0, 7
    N.lib().pfx_narf_desc_params_default(ctypes.byref(p))
    assert (p.support_size, p.rotation_invariant) == (-1.0, 1)
    N.lib().pfx_narf_desc_params_default(None)  # (a null pointer is ignored)
    assert ctypes.sizeof(N.NarfDescParams) == 8
    text = open(os.path.join(ROOT, "include", "pfx.h")).read()
    head, body = text.split("#ifndef PFX_H_")[0], text.split("#ifndef PFX_H_")[1]
    assert "pfx_narf_descriptors*" in head and "613-648" in head and "pfx_point_indices*" in head and "91-102" in head
    for stat in ("rows", "invalid_pixels", "pose_failed", "fallback_normals", "ring_max", "background_cells"):
        assert '"narf_desc_' + stat + '"' in body, stat


def test_python_signatures():
    import pcl_feature_extraction_amd as pkg
    from pcl_feature_extraction_amd import Context
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(pkg.narf_desc_params) == ["support_size", "rotation_invariant"]
    d = inspect.signature(pkg.narf_desc_params).parameters
    assert d["support_size"].default == 0.2 and d["rotation_invariant"].default is True
    assert params(Context.narf_descriptors) == ["self", "x", "y", "z", "pixel_idx", "params", "cam"]
    assert params(Context.point_indices) == ["self", "x", "y", "z", "kx", "ky", "kz", "tol"]
    assert inspect.signature(Context.point_indices).parameters["tol"].default == 1e-4
    assert params(Context.narf_descriptors_dev)[:5] == ["self", "x", "y", "z", "pixel_idx"]
    assert params(Context.point_indices_dev)[:7] == ["self", "x", "y", "z", "kx", "ky", "kz"]
    assert pkg.NarfDescriptors._fields == ("desc", "pose", "keypoint")
    assert {"narf_desc_params", "NarfDescriptors"} <= set(pkg.__all__)


# ---- on the GPU ----

def raw(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(ctypes.c_void_p)
    if isinstance(v, ctypes.Structure):
        return ctypes.byref(v)
    return ctypes.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The X ridge as a cloud: its centre pixel (four rows), a pixel beside it and a negative index;
    `keys`: the rows' entries by the restatement."""
    import narf_desc_ref as P
    from pcl_feature_extraction_amd import camera, narf_desc_params
    ri = K.depth_image(K.relief_depth(K.x_ridge), K.Q)
    x, y, z = K.image_cloud(ri)
    pix = np.array([K.Q_CENTRE, K.Q_CENTRE + 5 * 65 + 11, -1], np.int32)
    want = P.descriptors(P.build(tmp_path_factory.mktemp("narf_desc_ref")), x, y, z, pix, 0.2, True, K.Q)
    keys = want.keypoint.tolist()
    assert keys[:4] == [0, 0, 0, 0] and 5 <= len(keys) <= 9 and keys[-1] == 1
    return dict(x=x, y=y, z=z, pix=pix, cam=camera(**K.Q), prm=narf_desc_params(0.2), keys=keys)


def desc_forms(scene, cap):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda v: torch.tensor(v, device=dev)  # noqa: E731
    s = scene
    outs = [np.full((cap, 36), 7, np.float32), np.full((cap, 12), 7, np.float32), np.full(cap, -7, np.int32)]
    host = [s["x"], s["y"], s["z"], len(s["x"]), s["cam"], s["pix"], len(s["pix"]), s["prm"], *outs, cap,
            ctypes.c_int64(-7)]
    device = [up(v) if isinstance(v, np.ndarray) else v for v in host[:-1]] + [torch.full((1,), -7, dtype=torch.int64, device=dev)]
    torch.cuda.synchronize()
    return {"": host, "_dev": device}


def call(ctx, name, args):
    a = [ctypes.byref(v) if isinstance(v, ctypes.c_int64) else raw(v) for v in args]
    return getattr(ctx._lib, name)(ctx.h, *a)


def count_of(form, args):
    return args[-1].value if form == "" else int(args[-1].cpu().item())


@pytest.mark.gpu
def test_descriptor_argument_rule_of_both_forms(ctx, scene):
    from pcl_feature_extraction_amd import camera, narf_desc_params
    lib = ctx._lib
    m = len(scene["keys"])
    for form, args in desc_forms(scene, 15).items():
        name = "pfx_narf_descriptors" + form
        assert call(ctx, name, args) == N.PFX_OK, lib.pfx_last_error(ctx.h)
        ctx.synchronize()
        assert count_of(form, args) == m and ctx.stat("narf_desc_rows") == m and ctx.stat("narf_desc_invalid_pixels") == 1
        for i in (0, 1, 2, 4, 5, 7, 8, 9, 10, 12):  # the pointers
            b = list(args)
            b[i] = None
            assert call(ctx, name, b) == N.PFX_ERR_INVALID, (name, "null argument", i)
            assert lib.pfx_last_error(ctx.h).decode() == "narf_descriptors: invalid arguments", (name, i)
        for i in (3, 6, 11):
            b = list(args)
            b[i] = -1
            assert call(ctx, name, b) == N.PFX_ERR_INVALID, (name, "negative size", i)
        assert getattr(lib, name)(None, *[ctypes.byref(v) if isinstance(v, ctypes.c_int64) else raw(v) for v in args]) \
            == N.PFX_ERR_INVALID
        for support in (0.0, -1.0, float("nan")):
            b = list(args)
            b[7] = narf_desc_params(support)
            assert call(ctx, name, b) == N.PFX_ERR_INVALID, (name, support)
        default = N.NarfDescParams()
        lib.pfx_narf_desc_params_default(ctypes.byref(default))
        b = list(args)
        b[7] = default  # (support_size -1: must be set)
        assert call(ctx, name, b) == N.PFX_ERR_INVALID
        for bad in (dict(width=1025, height=64), dict(width=640, height=481), dict(width=0)):
            b[7], b[4] = scene["prm"], camera(**dict(K.Q, **bad))
            assert call(ctx, name, b) == N.PFX_ERR_INVALID, (name, bad)
        b[4] = camera(**dict(K.Q, noise_level=0.01))
        assert call(ctx, name, b) == N.PFX_ERR_UNSUPPORTED, name
        # nothing of the rejected calls was run: the statistics are the served call's
        ctx.synchronize()
        assert ctx.stat("narf_desc_rows") == m


@pytest.mark.gpu
def test_descriptor_capacity_and_empty_sides(ctx, scene):
    import torch
    rows, keys = {}, scene["keys"]
    m = len(keys)
    for cap in (m, m - 1):
        for form, args in desc_forms(scene, cap).items():
            code = call(ctx, "pfx_narf_descriptors" + form, args)
            ctx.synchronize()
            torch.cuda.synchronize()
            assert count_of(form, args) == m, (form, cap)
            desc, key = (args[8], args[10]) if form == "" else (args[8].cpu().numpy(), args[10].cpu().numpy())
            if cap == m:  # at the row count: served
                assert code == N.PFX_OK and key.tolist() == keys
                rows[form] = desc.copy()
            elif form == "":  # one below: the host form refuses, with the size needed, and writes nothing
                assert code == N.PFX_ERR_CAPACITY and (desc == 7).all() and (key == -7).all()
            else:  # the device form writes the first cap rows and the full count
                assert code == N.PFX_OK and key.tolist() == keys[:-1]
                assert np.array_equal(desc.view(np.uint32), rows["_dev"][:m - 1].view(np.uint32))
    assert np.array_equal(rows[""].view(np.uint32), rows["_dev"].view(np.uint32))
    for form, args in desc_forms(scene, m).items():
        name = "pfx_narf_descriptors" + form
        # nk == 0: null entry and output pointers and all; no row, nothing written
        b = list(args)
        b[5:7] = [None, 0]
        b[8:12] = [None, None, None, 0]
        assert call(ctx, name, b) == N.PFX_OK, form
        ctx.synchronize()
        assert count_of(form, args) == 0
        # n == 0: an empty image, every entry invalid
        b = list(args)
        b[0:4] = [None, None, None, 0]
        assert call(ctx, name, b) == N.PFX_OK, form
        ctx.synchronize()
        assert count_of(form, args) == 0 and ctx.stat("narf_desc_invalid_pixels") == 3 and ctx.stat("narf_desc_rows") == 0


@pytest.mark.gpu
def test_point_indices_rule_and_capacity(ctx):
    import torch
    dev = torch.device("cuda", 0)
    x = np.array([0, 1, 1, 2], np.float32)
    k = np.array([1, 2, 5], np.float32)  # -> 1, 2, 3
    for form in ("", "_dev"):
        name = "pfx_point_indices" + form
        up = (lambda v: torch.tensor(v, device=dev)) if form else (lambda v: v)  # noqa: E731

        def args(cap):
            n_out = torch.full((1,), -7, dtype=torch.int64, device=dev) if form else ctypes.c_int64(-7)
            a = [up(x), up(x), up(x), 4, up(k), up(k), up(k), 3, 1e-4, up(np.full(max(cap, 1), -7, np.int32)), cap, n_out]
            torch.cuda.synchronize()
            return a
        a = args(3)
        assert call(ctx, name, a) == N.PFX_OK
        ctx.synchronize()
        assert count_of(form, a) == 3 and (a[9] if form == "" else a[9].cpu().numpy()).tolist() == [1, 2, 3]
        for i in (0, 1, 2, 4, 5, 6, 9, 11):
            b = list(a)
            b[i] = None
            assert call(ctx, name, b) == N.PFX_ERR_INVALID, (name, i)
            assert ctx._lib.pfx_last_error(ctx.h).decode() == "point_indices: invalid arguments"
        for i, bad in ((3, -1), (7, -1), (10, -1), (8, float("nan")), (3, 1 << 31)):
            b = list(a)
            b[i] = bad
            assert call(ctx, name, b) == N.PFX_ERR_INVALID, (name, i, bad)
        a = args(2)  # one below the count
        code = call(ctx, name, a)
        ctx.synchronize()
        got = a[9] if form == "" else a[9].cpu().numpy()
        assert count_of(form, a) == 3
        if form == "":
            assert code == N.PFX_ERR_CAPACITY and got.tolist() == [-7, -7]
        else:
            assert code == N.PFX_OK and got.tolist() == [1, 2]
        for empty in (slice(0, 4), slice(4, 8)):  # n == 0, nk == 0: nothing matches
            a = args(3)
            a[empty] = [None, None, None, 0]
            assert call(ctx, name, a) == N.PFX_OK
            ctx.synchronize()
            assert count_of(form, a) == 0
