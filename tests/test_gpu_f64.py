"""GPU: the normals, FPFH-33 and SHOT-352 kernels against the float64 statements of
tests/f64_ref.py, on the clouds of tests/f64_cases.py and within the bounds of tests/f64_check.py
(the same constants the CPU restatement is held to in tests/test_f64_ref.py).

The bit-exact comparisons with the restatement (tests/test_gpu_features.py, tests/test_gpu_shot.py)
say that kernel and restatement agree; these say that what they agree on is the definition."""
import numpy as np
import pytest

import f64_cases as C
import f64_check as K
import f64_ref as R

pytestmark = pytest.mark.gpu


def _show(name, fig):
    print("\n%s: %s" % (name, ", ".join("%s %.3g" % kv for kv in fig.items())))


@pytest.mark.parametrize("case", [C.surface_origin, C.surface_range], ids=lambda f: f.__name__)
def test_normals_within_the_derived_bound(ctx, case):
    fig, _ = K.run_normals(ctx, case())
    _show(case.__name__ + " (worst angle, rad)", fig)


@pytest.mark.parametrize("case", [C.rough_blob, C.rough_blob_keypoints], ids=lambda f: f.__name__)
def test_fpfh_within_its_interval(ctx, case):
    fig, got = K.run_fpfh(ctx, case())
    _show(case.__name__, fig)
    if case is C.rough_blob_keypoints:
        assert np.isnan(got[-2:]).all() and np.isfinite(got[:-2]).all()


def _shot_and_lrf(ctx, c):
    fig, (desc, rf) = K.run_shot(ctx, c)
    # shot_lrf alone gives shot's frames bit for bit, so it is held to the same float64 frames
    lrf = ctx.shot_lrf(*K.xyz(c.P), *K.xyz(c.Q), c.r)
    assert np.array_equal(lrf.view(np.uint32), rf.view(np.uint32))
    use = K.shot_compared_rows(c.ref)
    assert K.shot_errors(c.ref, desc, lrf)[0][use].max() <= K.T_RF
    return fig


def test_shot_frame_and_descriptor(ctx):
    _show("aniso_blob", _shot_and_lrf(ctx, C.aniso_blob()))


def test_shot_long_list_next_to_split_lists(ctx):
    """dense_core: one query with more than 2,048 neighbours among 29 with fewer.  The split
    kernels (k_shot_lrf and what follows it, pfx_shot.hip) pass a list above their capacity
    (kCapSmall = 2,048, pfx_shot_core.h) on to the fused long-list kernel k_shot.  Two statistics
    of pfx_shot.hip show it: `shot_queued`, the number of queries passed on, is 1 with the dense
    query and 0 without it; `shot_neighbors`, to which either kernel adds the length of every
    list it finishes, equals the float64 neighbour counts, so every list was finished once."""
    c = C.dense_core()
    assert c.k[c.dense] > C.SPLIT_CAPACITY and (np.delete(c.k, c.dense) <= C.SPLIT_CAPACITY).all()
    _show("dense_core", _shot_and_lrf(ctx, c))
    ctx.shot(*K.xyz(c.P), *K.xyz(c.N), *K.xyz(c.Q), c.r)
    assert ctx.stat("shot_queued") == 1
    assert ctx.stat("shot_neighbors") == int(c.k.sum())
    short = np.arange(len(c.Q)) != c.dense
    desc, _ = ctx.shot(*K.xyz(c.P), *K.xyz(c.N), *K.xyz(c.Q[short]), c.r)
    assert ctx.stat("shot_queued") == 0
    assert ctx.stat("shot_neighbors") == int(c.k[short].sum())
    # and a list of exactly the capacity stays with the split kernels, one more leaves them: the
    # dense query's surface cut down to its 2,048 and 2,049 nearest points
    idx = R.neighbours(c.P, c.Q[c.dense], c.r)[0]
    for keep, queued in ((C.SPLIT_CAPACITY, 0), (C.SPLIT_CAPACITY + 1, 1)):
        P, N = c.P[idx[:keep]], c.N[idx[:keep]]
        desc, rf = ctx.shot(*K.xyz(P), *K.xyz(N), *K.xyz(c.Q[c.dense:c.dense + 1]), c.r)
        assert (ctx.stat("shot_queued"), ctx.stat("shot_neighbors")) == (queued, keep)
        rf64, (gap, x_margin, z_margin) = R.shot_lrf(P, c.Q[c.dense], c.r)
        assert gap >= C.SHOT_GAP_CASE and min(x_margin, z_margin) >= 1     # (0.028 and 1: the cut keeps the frame)
        assert np.abs(rf[0] - rf64).max() <= K.T_RF
        assert np.linalg.norm(desc[0] - R.shot352(P, N, c.Q[c.dense], rf64, c.r)) <= K.T_DESC


def test_chain_normals_fpfh_shot(ctx):
    fig, _ = K.run_chain(ctx, C.surface_chain())
    for stage, f in fig.items():
        _show("surface_chain " + stage, f)
