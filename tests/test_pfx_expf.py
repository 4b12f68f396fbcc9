"""pfx_expf (csrc/pfx_expf.h), the exponential of the intensity-spin contract, as g++ compiles it into
the restatement, against the host C library's expf.  Both are faithfully rounded, so they are never
more than 1 ulp apart; NaN, +-0, the cutoff to zero and the overflow agree exactly.  How often they
are 1 ulp apart is reported (pytest -s; DESIGN.md quotes it), not asserted: the header is the
contract, not the C library."""
import importlib.util
import os

import numpy as np
import pytest

import intensity_spin_ref as P
from parity import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pcl_feature_extraction_amd", "csrc", "pfx_expf.h")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("pfx_expf"))


def window(centre, half):
    """Every float within `half` bit patterns of centre (one sign)."""
    u = int(bits(np.float32(centre)).item())
    lo = max(u - half, u & 0x80000000)
    return np.arange(lo, u + half, dtype=np.uint32).view(np.float32)


WINDOWS = {
    "around +0": window(0.0, 1 << 18), "around -0": window(-0.0, 1 << 18),
    "around +2^-24": window(2.0 ** -24, 1 << 18), "around -2^-24": window(-(2.0 ** -24), 1 << 18),
    "around -1": window(-1.0, 1 << 18),
    "around -87.3 (the denormal threshold)": window(-87.3365, 1 << 18),
    "around -103.97 (the cutoff to zero)": window(-103.972, 1 << 18),
    "around 88.72 (the overflow)": window(88.7228, 1 << 18),
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_dense_windows_are_within_one_ulp_of_libm(ref, name):
    x = WINDOWS[name]
    hist, mismatch, worst = P.expf_compare(ref, x)
    print(f"pfx_expf vs libm expf, {name}: {len(x)} arguments, {hist[1]} are 1 ulp apart")
    assert hist.sum() == len(x) and hist[2] == 0, f"more than 1 ulp apart at {worst!r}"
    assert mismatch == 0


def test_a_seeded_million_is_within_one_ulp_of_libm(ref):
    x = np.random.default_rng(2718).uniform(-110.0, 10.0, 1000000).astype(np.float32)
    hist, mismatch, worst = P.expf_compare(ref, x)
    print(f"pfx_expf vs libm expf, 1,000,000 seeded arguments in [-110, 10]: {hist[1]} are 1 ulp apart")
    assert hist.sum() == len(x) and hist[2] == 0, f"more than 1 ulp apart at {worst!r}"
    assert mismatch == 0


def test_special_values(ref):
    b = lambda x: int(bits(P.expf(ref, x)).item())  # noqa: E731
    assert b(np.nan) == 0x7fc00000 and np.isnan(P.libm_expf(ref, np.nan))
    assert b(0.0) == b(-0.0) == int(bits(np.float32(1.0)).item())
    assert b(-np.inf) == 0 and b(np.inf) == 0x7f800000
    f32max = float(np.finfo(np.float32).max)
    assert b(-f32max) == 0 and b(f32max) == 0x7f800000
    # the cutoff: e^x <= 2^-150 rounds to +0, above it to the smallest denormal
    assert b(-103.98) == 0 and b(-103.97) == 1
    # a denormal result comes from the one conversion: e^-95 = 2^-137.06 has 13 bits left
    assert 0 < b(-95.0) < 0x00800000 and abs(b(-95.0) - int(bits(P.libm_expf(ref, -95.0)).item())) <= 1
    assert abs(b(-95.0) * 2.0 ** -149 / np.exp(-95.0) - 1.0) < 2.0 ** -13
    # positive arguments are right too, up to the overflow
    assert P.expf(ref, 1.0) == np.float32(np.e) and abs(b(88.72) - int(bits(P.libm_expf(ref, 88.72)).item())) <= 1
    assert np.isinf(P.expf(ref, 88.73)) and np.isinf(P.libm_expf(ref, 88.73))
    specials = np.float32([np.nan, 0.0, -0.0, np.inf, -np.inf, f32max, -f32max, 89.0, 89.5, -104.0, -104.5, -103.99])
    hist, mismatch, _ = P.expf_compare(ref, specials)
    assert mismatch == 0 and hist[2] == 0


def test_the_header_holds_the_generators_constants():
    """scripts/pfx_expf_table.py rounds the constants from 50 decimal digits; the header's literals are
    its output."""
    spec = importlib.util.spec_from_file_location("pfx_expf_table", os.path.join(ROOT, "scripts", "pfx_expf_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    c = gen.constants()
    with open(HEADER) as f:
        text = f.read()
    for v in c["table"]:
        assert "0x%016xull" % v in text
    for name in ("inv_ln2_n", "c1", "c2", "c3"):
        assert "0x%016xull" % gen.bits(c[name]) in text, name
    assert c["table"][0] == 0x3ff0000000000000 and len(c["table"]) == 32
