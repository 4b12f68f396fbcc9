"""The moment-invariant and principal-curvature boundary, without a GPU: the four C symbols are
declared in include/pfx.h, exported by libpfx.so and bound with the header's argument lists, and the
Python front-end has the signatures the issue states."""
import ctypes
import inspect
import os
import re

from pcl_feature_extraction_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pfx_moment_invariants", "pfx_moment_invariants_dev", "pfx_principal_curvatures",
           "pfx_principal_curvatures_dev")


def _prototypes():
    src = open(os.path.join(ROOT, "include", "pfx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"pfx_status\s+(pfx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_symbols_declared_exported_and_bound():
    protos, lib = _prototypes(), N.lib()
    kinds = {"pfx_ctx*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
             "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    for name in SYMBOLS:
        assert name in protos and hasattr(lib, name) and name in N.exported_symbols(), name
        want = [kinds[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in protos[name]]
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 or fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want, name
    names = lambda f: [a.split()[-1].lstrip("*") for a in protos[f]]  # noqa: E731
    assert names("pfx_moment_invariants") == ["ctx", "sx", "sy", "sz", "n_surface", "qx", "qy", "qz", "nq", "radius",
                                              "out"]
    assert names("pfx_principal_curvatures") == ["ctx", "sx", "sy", "sz", "snx", "sny", "snz", "n_surface", "qx", "qy",
                                                 "qz", "qnx", "qny", "qnz", "nq", "radius", "out"]
    for f in ("pfx_moment_invariants", "pfx_principal_curvatures"):
        assert [a.replace("d_", "") for a in names(f + "_dev")] == names(f)


def test_header_names_the_replaced_interfaces():
    text = open(os.path.join(ROOT, "include", "pfx.h")).read()
    head = text.split("#ifndef PFX_H_")[0]
    assert "pfx_moment_invariants*" in head and "MomentInvariantsEstimation" in head and "554-572" in head
    assert "pfx_principal_curvatures*" in head and "PrincipalCurvaturesEstimation" in head and "696-715" in head
    body = text.split("#ifndef PFX_H_")[1]
    for stat in ("moments_neighbors", "moments_kmax", "moments_queued", "pcurv_neighbors", "pcurv_kmax", "pcurv_queued",
                 "moments_cap_small"):
        assert '"' + stat + '"' in body, stat


def test_python_signatures():
    from pcl_feature_extraction_amd import Context
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(Context.moment_invariants) == ["self", "sx", "sy", "sz", "qx", "qy", "qz", "r"]
    assert params(Context.moment_invariants_dev) == ["self", "sx", "sy", "sz", "qx", "qy", "qz", "r", "out"]
    assert params(Context.principal_curvatures) == ["self", "sx", "sy", "sz", "snx", "sny", "snz", "qx", "qy", "qz",
                                                    "qnx", "qny", "qnz", "r"]
    assert params(Context.principal_curvatures_dev) == ["self", "sx", "sy", "sz", "snx", "sny", "snz", "qx", "qy", "qz",
                                                        "qnx", "qny", "qnz", "r", "out"]


def test_facade_declares_the_point_types_and_estimators():
    hpp = open(os.path.join(ROOT, "include", "pfx_pcl.hpp")).read()
    assert re.search(r"class MomentInvariantsEstimation : public Feature<PointInT, PointOutT>", hpp)
    assert re.search(r"class PrincipalCurvaturesEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT>", hpp)
    assert "DescriptorLayout<MomentInvariants> { static constexpr int dim = 3, stride = 3; }" in hpp
    assert "DescriptorLayout<PrincipalCurvatures> { static constexpr int dim = 3, stride = 5; }" in hpp
