"""Fitness of the inputs of tests/test_gpu_match_bound.py, proved on the CPU with the NumPy model
of the matcher's bound pass (tests/match_model.py) against the oracle (oracle/or_match.cpp).

These are conditions on the INPUTS, not measurements of the kernel: they are what keeps the GPU
parity test from being toothless.  The model as written must keep every oracle minimiser and stay
inside its own error bound; the model with a defect a kernel edit could introduce (a low part of
the bf16 split dropped from the packed product, a norm that misses a dimension) must lose a
minimiser, at every descriptor width; pruning must be a real decision (several candidates per
row) and, on one input, impossible.  If an input fails a condition, change the input."""
import functools

import numpy as np
import pytest

import match_model as mm
import oracle_lib as O
from match_data import BOUND_CASES, bound_case, overflow_fallback_pair, overflow_pair, scaled_pair

SMALL = [n for n in BOUND_CASES if n.startswith(("offset", "coherent")) and BOUND_CASES[n][1][1] <= 300]
WIDTHS = (33, 125, 352, 1344)


def _width(name):
    return BOUND_CASES[name][1][0]


@functools.lru_cache(maxsize=None)
def _input(name):
    if name in BOUND_CASES:
        src, tgt = bound_case(name)
    else:
        src, tgt = {"tiny": lambda: scaled_pair(-70), "huge": lambda: scaled_pair(40), "overflow": overflow_pair,
                    "overflow_fallback": overflow_fallback_pair}[name]()
    s2t, _ = O.nearest_descriptor(src, tgt)
    t2s, _ = O.nearest_descriptor(tgt, src)
    return src, tgt, mm.l2_simple_all(src, tgt), s2t, t2s


@functools.lru_cache(maxsize=None)
def _model(name, mutant):
    src, tgt, l2, s2t, t2s = _input(name)
    return mm.bound_pass(src, tgt, mutant, l2=l2, s2t=s2t, t2s=t2s)


def test_bf16_split_is_the_kernels():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.1415927, 1e-30, 65504.0, 0.1], np.float32)
    # 1 + 2^-8 is a tie: to even (down); 1 + 3 2^-8 is a tie: to even (up)
    assert list(mm.bf16_rne(x[:3])) == [0x3F80, 0x3F80, 0x3F82]
    hi, lo = mm.split(x)
    rest = x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert np.all(np.abs(rest) <= 2.0 ** -16 * np.abs(x.astype(np.float64)) + 1e-45)
    assert np.array_equal(mm.bf16_round(hi), hi) and np.array_equal(mm.bf16_round(lo), lo)


@pytest.mark.parametrize("name", list(BOUND_CASES) + ["tiny", "huge", "overflow", "overflow_fallback"])
def test_model_keeps_every_minimiser_within_its_bound(name):
    src, tgt, l2, s2t, t2s = _input(name)
    # (the model's own L2_Simple is the oracle's: the same minimisers, lowest row on ties)
    assert np.array_equal(np.argmin(l2, axis=1), s2t) and np.array_equal(np.argmin(l2, axis=0), t2s)
    r = _model(name, "none")
    print("%s: candidates/row %.2f, max |dh - L2| / e %.4f" % (name, r.cand_per_row, r.max_ratio))
    assert r.lost == 0
    assert r.max_ratio <= 1.0
    if name in BOUND_CASES:  # a tie would make "lost" ambiguous
        assert len(r.tied_rows) == 0 and len(r.tied_cols) == 0


def test_magnitude_edge_inputs_are_what_they_claim():
    src, tgt, l2, s2t, t2s = _input("tiny")
    tiny = np.finfo(np.float32).tiny
    # every squared difference is subnormal, and so is every distance the matcher reports (the
    # largest distances of the full matrix, sums of 33 of them, reach 1.3 x the smallest normal)
    d = src[:, None, :].astype(np.float64) - tgt[None, :, :]
    assert (d * d).max() < tiny
    near = np.concatenate([l2.min(axis=1), l2.min(axis=0)])
    assert near.max() < tiny and near.min() > 0 and np.median(l2) < tiny
    hs, ht, hl2 = _input("huge")[:3]
    assert np.isfinite(hl2).all() and mm.norm2_fp32(hs).max() > 1e27
    # powers of two scale the oracle's distances exactly
    base = _input("huge")[2] * np.float32(2.0) ** np.float32(-80)
    os, ot = scaled_pair(0)
    assert np.array_equal(mm.l2_simple_all(os, ot), base)
    src, tgt, l2, s2t, t2s = _input("overflow")
    assert np.isfinite(src).all() and np.isfinite(tgt).all()
    assert np.isinf(mm.norm2_fp32(src)[[3, 140]]).all() and np.isinf(mm.norm2_fp32(tgt)[[9, 200]]).all()
    assert s2t[3] == 9 and t2s[9] == 3 and l2[3, 9] == 0.0
    assert np.isinf(l2[140]).all() and s2t[140] == 0
    assert np.isinf(l2[:, 200]).all() and t2s[200] == 0
    src, tgt, l2, s2t, t2s = _input("overflow_fallback")
    assert np.isfinite(src).all() and np.isfinite(tgt).all()
    assert s2t[3] == 9 and t2s[9] == 3 and np.isinf(l2[140]).all() and np.isinf(l2[:, 200]).all()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mutant", ["no_alo", "no_blo", "nolo"])
def test_a_dropped_low_part_loses_a_minimiser_at_every_width(width, mutant):
    lost = {n: _model(n, mutant).lost for n in SMALL if _width(n) == width}
    print(mutant, lost)
    assert lost and max(lost.values()) >= 1


def test_a_short_norm_loses_a_minimiser():
    lost = {n: _model(n, "n2_tail").lost for n in SMALL}
    print(lost)
    assert max(lost.values()) >= 1


def test_pruning_is_a_real_decision():
    for width in WIDTHS:
        assert max(_model(n, "none").cand_per_row for n in SMALL if _width(n) == width) >= 2.0
    assert any(_model(n, "none").all_candidates for n in SMALL)
