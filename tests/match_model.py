"""NumPy model of the matcher's bound pass (pfx_match.hip: prep + bound + prune) -- TEST
INFRASTRUCTURE ONLY.  It decides whether an input makes pruning a real decision, and whether a
kernel with a plausible defect would lose a true nearest row on it.

Modelled, in the kernel's arithmetic: bf16 round-to-nearest-even, hi = bf16(v) and
lo = bf16(v - hi), the packed three-term product a_hi.b_hi + a_hi.b_lo + a_lo.b_hi, the fp32
squared norm (64 lane partial sums + the xor butterfly, no FMA) and its fp32 square root,
dh = (n2a + n2b) - 2 dot, e = 1.5 (c1 (|a| + |b|)^2 + c2 |a||b|) + 1e-30 with the host's c1 and c2,
U_row / U_col = min max(dh + e, 0), lb = dh - e, the candidate sets lb <= U, and the rule that a
pair whose dh or e is not finite is unbounded and unprunable (ub = +inf, lb = -inf).

NOT modelled: the MFMA's accumulation order.  The model accumulates the split product in
float64 and rounds once to fp32; the kernel's e is meant to cover whatever order (and
truncation) the matrix cores use, and max |dh - L2_Simple| / e of the model says how much room
that leaves.  Rows are assumed finite (the kernel's validity flag is not modelled).

mutant= breaks the model the way a kernel edit could:
  "none"     the kernel as written
  "no_alo"   the packed product lacks a_lo.b_hi
  "no_blo"   the packed product lacks a_hi.b_lo
  "nolo"     it lacks both low parts
  "n2_tail"  the source rows' squared norm misses the last dimension
"""
import numpy as np

MUTANTS = ("none", "no_alo", "no_blo", "nolo", "n2_tail")


def bf16_rne(x):
    """float32 -> bf16 bits, round to nearest even, as k_match_prep's bf16_rne."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_val(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(x):
    """float32 -> the nearest bf16 value, as float32."""
    return bf16_val(bf16_rne(x))


def split(x):
    """(hi, lo) of every element: hi = bf16(v), lo = bf16(v - hi) (the difference is exact)."""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def norm2_fp32(x):
    """k_match_prep's squared norm: lane k % 64 adds v*v in turn, then the xor butterfly."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    pad = np.zeros((n, (d + 63) // 64 * 64), np.float32)
    pad[:, :d] = x
    part = np.zeros((n, 64), np.float32)
    lanes = np.arange(64)
    with np.errstate(over="ignore"):
        for c in range(0, pad.shape[1], 64):
            blk = pad[:, c:c + 64]
            part = part + blk * blk
        for o in (32, 16, 8, 4, 2, 1):
            part = part + part[:, lanes ^ o]
    return part[:, 0].copy()


def l2_simple_all(a, b):
    """FLANN L2_Simple<float> of every pair: sequential fp32 adds over the dimensions."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    r = np.zeros((len(a), len(b)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(a.shape[1]):
            d = a[:, k, None] - b[None, :, k]
            d *= d
            r += d
    return r


def coefficients(d):
    """c1, c2 of e as match_nearest_dev evaluates them in fp32."""
    f = np.float32
    u = f(5.9604645e-8)
    c1 = (f(2.0) * f(d) + f(6.1)) * u
    c2 = f(12.2) * f(d) * u + f(6.2) / f(65536.0)
    return f(c1), f(c2)


class BoundResult:
    """lost_rows / lost_cols: rows (columns) whose minimiser is not a candidate; cand_per_row:
    mean row candidates; all_candidates: no pair pruned; max_ratio: largest |dh - L2| / e over
    the pairs with finite dh and e; tied_rows / tied_cols: rows (columns) whose minimal L2_Simple
    occurs more than once."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def lost(self):
        return len(self.lost_rows) + len(self.lost_cols)


def bound_pass(src, tgt, mutant="none", l2=None, s2t=None, t2s=None):
    """One bound pass of the model.  l2: l2_simple_all(src, tgt) when the caller has it;
    s2t / t2s: the minimisers to look for (default: the first minimum of l2 each way)."""
    assert mutant in MUTANTS
    src = np.ascontiguousarray(src, np.float32)
    tgt = np.ascontiguousarray(tgt, np.float32)
    d = src.shape[1]
    if l2 is None:
        l2 = l2_simple_all(src, tgt)
    if s2t is None:
        s2t = np.argmin(l2, axis=1)
    if t2s is None:
        t2s = np.argmin(l2, axis=0)
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        ah, al = (x.astype(np.float64) for x in split(src))
        bh, bl = (x.astype(np.float64) for x in split(tgt))
        dot = ah @ bh.T
        if mutant not in ("no_blo", "nolo"):
            dot = dot + ah @ bl.T
        if mutant not in ("no_alo", "nolo"):
            dot = dot + al @ bh.T
        dot = dot.astype(np.float32)
        n2a = norm2_fp32(src[:, :-1] if mutant == "n2_tail" else src)
        n2b = norm2_fp32(tgt)
        nra, nrb = np.sqrt(n2a), np.sqrt(n2b)  # fp32, correctly rounded as sqrtf
        c1, c2 = coefficients(d)
        dh = (n2a[:, None] + n2b[None, :]) - f(2.0) * dot
        s = nra[:, None] + nrb[None, :]
        e = f(1.5) * (c1 * (s * s) + c2 * (nra[:, None] * nrb[None, :])) + f(1e-30)
        fin = (np.abs(dh) + e) < f(np.inf)
        ub = np.where(fin, np.maximum(dh + e, f(0.0)), f(np.inf))
        lb = np.where(fin, dh - e, f(-np.inf))
        # the kernel's running bounds start at 0x7f7f7f7f and only ever take a ub < +inf
        top = np.array([0x7F7F7F7F], np.uint32).view(np.float32)[0]
        u_row = np.minimum(ub.min(axis=1), top)
        u_col = np.minimum(ub.min(axis=0), top)
        crow = lb <= u_row[:, None]
        ccol = lb <= u_col[None, :]
        ok = fin & np.isfinite(l2)
        ratio = np.abs(dh.astype(np.float64) - l2.astype(np.float64)) / e.astype(np.float64)
        bad = fin & ~np.isfinite(l2)  # a finite bound on a non-finite distance is no bound
        max_ratio = float(ratio[ok].max()) if ok.any() else 0.0
        if bad.any():
            max_ratio = float("inf")
    rows, cols = np.arange(len(src)), np.arange(len(tgt))
    mn_r, mn_c = l2.min(axis=1), l2.min(axis=0)
    return BoundResult(
        lost_rows=rows[~crow[rows, s2t]], lost_cols=cols[~ccol[t2s, cols]],
        cand_per_row=float(crow.sum()) / len(src), cand_per_col=float(ccol.sum()) / len(tgt),
        all_candidates=bool(crow.all()), max_ratio=max_ratio,
        tied_rows=rows[(l2 == mn_r[:, None]).sum(axis=1) > 1],
        tied_cols=cols[(l2 == mn_c[None, :]).sum(axis=0) > 1],
        s2t=np.asarray(s2t), t2s=np.asarray(t2s))


if __name__ == "__main__":  # the table of DESIGN.md's matching section
    from match_data import BOUND_CASES, bound_case
    print("| input | rows | cand/row | max abs(dh-L2)/e | lost " + " | lost ".join(MUTANTS[1:]) + " |")
    print("|---|---|---|---|" + "---|" * len(MUTANTS[1:]))
    for name in BOUND_CASES:
        a, b = bound_case(name)
        full = l2_simple_all(a, b)
        res = [bound_pass(a, b, m, l2=full) for m in MUTANTS]
        assert res[0].lost == 0
        print("| %s | %d x %d | %.2f | %.3f | %s |" % (name, len(a), len(b), res[0].cand_per_row, res[0].max_ratio,
                                                     " | ".join(str(r.lost) for r in res[1:])))
