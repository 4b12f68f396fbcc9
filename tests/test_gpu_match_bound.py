"""GPU parity of the descriptor matcher where its pruning bound decides the answer, and at the
edges of the fp32 range -- against the CPU restatement (oracle/or_match.cpp), bit-exact: both
directions, indices, distance bits, correspondences (match_gpu._check).

The matcher's exactness rests on an argument (pfx_match.hip header): a bf16-split contraction
gives d^, an analytic e bounds |d^ - L2_Simple|, and every pair with d^ - e above the row's and
the column's bound is pruned before the exact pass.  A defect in the split, the packing order,
the norms, e or the prune test prunes the true nearest row silently, and only an input on which
pruning is a real decision shows it.  tests/test_match_model.py proves on the CPU that these
inputs are such: the model of the bound pass keeps several candidates per row on them (all of
them on one), and loses minimisers as soon as a low part of the split or a dimension of the norm
is dropped -- at every descriptor width (33, 125, 352, 1344).

Which inputs overflow the pruned pair list (the two-contraction fallback): test_bound_parity's
docstring."""
import numpy as np
import pytest

import oracle_lib as O
from match_data import (BOUND_CASES, OVERFLOW_SRC, OVERFLOW_TGT, bound_case, overflow_fallback_pair, overflow_pair,
                        scaled_pair)
from match_gpu import _check, _gpu_nearest, _same

pytestmark = pytest.mark.gpu


def _report(ctx, name):
    print("%s: pairs emitted %d (cap %d), candidates rows %d cols %d" % (
        name, ctx.stat("match_pairs_emitted"), ctx.stat("match_pair_cap"), ctx.stat("match_candidates_rows"),
        ctx.stat("match_candidates_cols")))


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_bound_parity(ctx, name):
    """Offset and coherent inputs at 300 x 280 / 300 x 300 (D = 125 through the scalar L2_Simple
    path, D = 352 and 1344 through the 16-byte one; the first multi-tile runs of D = 125 and 1344),
    the offset input over the seeding cross (2200 x 2300), and strongly unequal tile grids
    (2600 x 40, 40 x 2600, and 1153 x 1025 = 10 x 9 tiles: not a multiple of the 8-tile row group).

    Pair-list overflow, observed on an MI355X (recorded, not asserted): only offset33_s1_10x9
    overflows the pruned pair list (1,088,507 pairs emitted against a cap of 204,928; 295,679 row
    candidates) and takes the two-contraction fallback, a path otherwise reached only through
    exact duplicates.  The 300 x 280 inputs cannot overflow whatever their sigma: the cap,
    64 (ns + nt) + 65536 = 102,656, exceeds their 84,000 pairs -- offset33_s03 emits all 84,000
    and offset125_s01 83,951, and the emitting pass alone serves them.  The GPU's candidate
    counts equal the model's (offset33_s3: 523 row candidates = 1.74 x 300)."""
    src, tgt = bound_case(name)
    s2t, _, _, _ = _gpu_nearest(ctx, src, tgt)
    _report(ctx, name + " (nearest)")
    n = _check(ctx, src, tgt)
    _report(ctx, name + " (correspondences)")
    assert n > 0
    assert ctx.stat("match_candidates_rows") >= np.count_nonzero(s2t >= 0)


@pytest.mark.parametrize("exp", [-70, 40])
def test_scaled_by_a_power_of_two(ctx, exp):
    """An fpfh pair times 2^-70 (every squared difference and every reported distance is
    subnormal: the build keeps fp32 denormals, and the matcher must too) and times 2^40 (squared
    norms near 1e28).  The scaling is exact, so the matches are those of the unscaled pair and
    the distances its distances times 2^(2 exp) while they are normal numbers."""
    src, tgt = scaled_pair(exp)
    n = _check(ctx, src, tgt)
    _report(ctx, "2^%d" % exp)
    base_s, base_t = scaled_pair(0)
    assert n == len(O.correspondences(base_s, base_t)[0])
    s2t, ds, _, _ = _gpu_nearest(ctx, src, tgt)
    assert ctx.stat("match_candidates_rows") >= np.count_nonzero(s2t >= 0)
    if exp > 0:
        bs2t, bds = O.nearest_descriptor(base_s, base_t)
        assert np.array_equal(s2t, bs2t) and _same(ds, bds * np.float32(2.0) ** np.float32(2 * exp))
    else:
        assert 0 < ds.min() and ds.max() < np.finfo(np.float32).tiny


def test_finite_rows_whose_squared_norm_overflows(ctx):
    """pfx.h: only a non-finite VALUE leaves a row unmatched.  Source rows 3, 140 and target rows
    9, 200 are finite with |row|^2 = +inf in fp32; target row 9 equals source row 3 (distance 0, a
    mutual match); source row 140 and target row 200 have only +inf distances, so the oracle gives
    them the lowest finite row of the other side and distance +inf.  The other rows must match as
    if the four were not special."""
    src, tgt = overflow_pair()
    s2t, ds, t2s, dt = _gpu_nearest(ctx, src, tgt)
    _report(ctx, "overflow")
    os2t, ods = O.nearest_descriptor(src, tgt)
    ot2s, odt = O.nearest_descriptor(tgt, src)
    rest_s = np.setdiff1d(np.arange(len(src)), OVERFLOW_SRC)
    rest_t = np.setdiff1d(np.arange(len(tgt)), OVERFLOW_TGT)
    print("scaled source rows:", s2t[list(OVERFLOW_SRC)], ds[list(OVERFLOW_SRC)], "oracle", os2t[list(OVERFLOW_SRC)],
          ods[list(OVERFLOW_SRC)])
    print("scaled target rows:", t2s[list(OVERFLOW_TGT)], dt[list(OVERFLOW_TGT)], "oracle", ot2s[list(OVERFLOW_TGT)],
          odt[list(OVERFLOW_TGT)])
    assert np.array_equal(s2t[rest_s], os2t[rest_s]) and _same(ds[rest_s], ods[rest_s])
    assert np.array_equal(t2s[rest_t], ot2s[rest_t]) and _same(dt[rest_t], odt[rest_t])
    assert s2t[3] == 9 and ds[3] == 0.0 and t2s[9] == 3 and dt[9] == 0.0
    assert s2t[140] == 0 and ds[140] == np.inf
    assert t2s[200] == 0 and dt[200] == np.inf
    assert ctx.stat("match_candidates_rows") >= len(src)
    _check(ctx, src, tgt)
    q, m = ctx.correspondences(src, tgt)
    assert m[list(q).index(3)] == 9


def test_overflowing_norms_through_the_fallback(ctx):
    """The same four rows in the 1153 x 1025 offset input, whose pair list overflows: the
    two-contraction fallback must treat non-finite bounds as the emitting pass does."""
    src, tgt = overflow_fallback_pair()
    s2t, ds, t2s, dt = _gpu_nearest(ctx, src, tgt)
    _report(ctx, "overflow + fallback")
    assert ctx.stat("match_pairs_emitted") > ctx.stat("match_pair_cap") > 0
    assert s2t[3] == 9 and ds[3] == 0.0 and t2s[9] == 3 and dt[9] == 0.0
    assert s2t[140] == 0 and ds[140] == np.inf and t2s[200] == 0 and dt[200] == np.inf
    _check(ctx, src, tgt)
    assert ctx.stat("match_candidates_rows") >= len(src)
