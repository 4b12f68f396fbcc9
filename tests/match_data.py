"""Synthetic descriptor sets for the matching tests (Features<T>::findCorrespondences,
features.h:224-253): FPFH-like rows (three 11-bin blocks, each summing to 100, as
FPFHEstimation::computeFeature normalises them) and SHOT-like rows (352 non-negative values,
unit L2 norm, as SHOTEstimation normalises them), with a target that is a perturbed permutation
of the source plus distractors -- so most rows have a clear mutual nearest neighbour and some
rows are ambiguous."""
import numpy as np


def fpfh_like(rng, n):
    x = rng.gamma(0.6, 1.0, size=(n, 33)).astype(np.float64)
    for b in range(3):
        blk = x[:, 11 * b:11 * b + 11]
        x[:, 11 * b:11 * b + 11] = blk * (100.0 / blk.sum(1, keepdims=True))
    return x.astype(np.float32)


def shot_like(rng, n, d=352):
    x = rng.gamma(0.3, 1.0, size=(n, d)) * (rng.random((n, d)) < 0.4)
    x[:, 0] += 1e-3
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def pair(kind, ns, nt, seed, noise=0.02):
    rng = np.random.default_rng(seed)
    make = fpfh_like if kind == "fpfh" else shot_like
    src = make(rng, ns)
    m = min(ns, nt) * 3 // 4
    perm = rng.permutation(ns)[:m]
    scale = 100.0 if kind == "fpfh" else 1.0 / 16
    tgt = np.concatenate([src[perm] + (rng.normal(0, noise * scale, (m, src.shape[1]))).astype(np.float32),
                          make(rng, nt - m)])
    order = rng.permutation(nt)
    return src, np.ascontiguousarray(tgt[order]).astype(np.float32)


def offset_pair(d, ns, nt, seed, off, sigma):
    """Rows = a common vector c (uniform in [0, off)^d) + N(0, sigma) noise; the first
    3 min(ns, nt) / 4 target rows are permuted source rows + N(0, 0.1 sigma), the rest fresh rows,
    in shuffled order.  Every distance is tiny against (|a| + |b|)^2, so the matcher's
    d^ = |a|^2 + |b|^2 - 2 a.b is pure cancellation: sigma moves the input from "the pruning bound
    decides" to "nothing can be pruned"."""
    rng = np.random.default_rng(seed)
    c = rng.random(d) * off
    src = (c + rng.normal(0, sigma, (ns, d))).astype(np.float32)
    m = 3 * min(ns, nt) // 4
    perm = rng.permutation(ns)[:m]
    tgt = np.concatenate([src[perm] + rng.normal(0, 0.1 * sigma, (m, d)).astype(np.float32),
                          (c + rng.normal(0, sigma, (nt - m, d))).astype(np.float32)])
    order = rng.permutation(nt)
    return src, np.ascontiguousarray(tgt[order]).astype(np.float32)


def coherent_pair(d, k, v, seed, d2):
    """k SHOT-like vectors G, v variants of each on either side (k v rows a side, shuffled).  A
    variant is bf16(|G + N(0, sqrt(d2 / d))|) (1 +- 2^-9), the sign drawn per row: the product is
    exact in fp32, the bf16 high part of every element is the bf16 value and the low part is
    +-2^-9 of it with the row's sign -- so the split's low parts add up over d instead of averaging
    out, which random rows of this width never make them do."""
    from match_model import bf16_round
    rng = np.random.default_rng(seed)
    g = shot_like(rng, k, d=d)

    def side():
        x = np.repeat(g, v, axis=0) + rng.normal(0, np.sqrt(d2 / d), (k * v, d))
        x = bf16_round(np.abs(x).astype(np.float32))
        sign = np.where(rng.random(k * v) < 0.5, -1.0, 1.0)
        x = x * (1.0 + sign * 2.0 ** -9).astype(np.float32)[:, None]
        return np.ascontiguousarray(x[rng.permutation(k * v)]).astype(np.float32)

    src = side()
    return src, side()


# The inputs of tests/test_gpu_match_bound.py, whose fitness tests/test_match_model.py proves on
# the CPU: name -> (builder, arguments).  (dimension, family) is read off the name.
BOUND_CASES = {
    "offset33_s3": (offset_pair, (33, 300, 280, 2, 100.0, 3.0)),
    "offset33_s1": (offset_pair, (33, 300, 280, 2, 100.0, 1.0)),
    "offset33_s03": (offset_pair, (33, 300, 280, 2, 100.0, 0.3)),
    "offset125_s03": (offset_pair, (125, 300, 280, 2, 10.0, 0.3)),
    "offset125_s01": (offset_pair, (125, 300, 280, 2, 10.0, 0.1)),
    "coherent33": (coherent_pair, (33, 100, 3, 5, 1e-3)),
    "coherent125": (coherent_pair, (125, 100, 3, 5, 1e-3)),
    "coherent352": (coherent_pair, (352, 100, 3, 5, 1e-3)),
    "coherent1344": (coherent_pair, (1344, 100, 3, 5, 1e-3)),
    "offset33_s3_cross": (offset_pair, (33, 2200, 2300, 2, 100.0, 3.0)),
    "fpfh_tall": (pair, ("fpfh", 2600, 40, 2640)),
    "fpfh_wide": (pair, ("fpfh", 40, 2600, 2640)),
    "offset33_s1_10x9": (offset_pair, (33, 1153, 1025, 2, 100.0, 1.0)),
}


def bound_case(name):
    make, args = BOUND_CASES[name]
    return make(*args)


def scaled_pair(exp):
    """pair("fpfh", 300, 280) times 2^exp: a power of two, so every L2_Simple distance scales
    exactly (until it leaves the normal range)."""
    src, tgt = pair("fpfh", 300, 280, seed=580)
    s = np.float32(2.0) ** np.float32(exp)
    return src * s, tgt * s


OVERFLOW_SRC, OVERFLOW_TGT = (3, 140), (9, 200)


def overflow_pair():
    """Finite rows whose squared norm overflows fp32: source rows 3 and 140 and target rows 9 and
    200 of a normal fpfh pair times 2^62; target row 9 = source row 3 (distance 0: a mutual
    match), source row 140 and target row 200 have only infinite distances."""
    src, tgt = pair("fpfh", 300, 280, seed=580)
    big = np.float32(2.0) ** np.float32(62)
    for r in OVERFLOW_SRC:
        src[r] *= big
    for r in OVERFLOW_TGT:
        tgt[r] *= big
    tgt[OVERFLOW_TGT[0]] = src[OVERFLOW_SRC[0]]
    return src, tgt


def overflow_fallback_pair():
    """The same four overflowing rows in the 1153 x 1025 offset input, whose pair list overflows:
    the non-finite bounds through the two-contraction fallback."""
    src, tgt = bound_case("offset33_s1_10x9")
    big = np.float32(2.0) ** np.float32(62)
    for r in OVERFLOW_SRC:
        src[r] *= big
    for r in OVERFLOW_TGT:
        tgt[r] *= big
    tgt[OVERFLOW_TGT[0]] = src[OVERFLOW_SRC[0]]
    return src, tgt
