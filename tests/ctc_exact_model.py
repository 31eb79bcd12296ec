"""Float64 references of the CTC cost and gradient (ctc_fast.pyx:13-152) whose forward-backward product cannot
underflow (no tests here: tests/test_ctc_exact_model_cpu.py checks them, tests/test_gpu_ctc_lazy.py uses them).

The recursion is the one of tests/test_ctc_store_model.lattice, but a row is never divided by its band sum.  Two
forms, `exact(..., rows=)`:

  "row"      every row is rescaled by an exact power of two (frexp of its largest element, ldexp) and its integer
             exponent is carried beside it, so the rescaling rounds nothing.  WITHIN a row this is the reference's
             arithmetic: a state more than 2^1074 below the row's largest is flushed to zero, as it is in the
             reference's sum-normalised rows (and in every kernel here: they all keep float64 rows scaled per frame).
  "element"  every element is a float64 mantissa in [0.5, 1) with its own integer exponent; the three terms of a
             transition are added on the largest one's exponent.  Nothing is ever flushed: this is the CTC likelihood
             itself (a log-space recursion gives the same cost to 1e-15).

In both the cost is the last row's exponent * ln 2 plus ONE logarithm, of that row's mass, and for the gradient the
product alpha_t[s] * beta_t[s] is formed from the two mantissas with the two exponents added BEFORE the product is
scaled back (relative to the frame's largest product): it underflows only where it is 2^-1074 below the frame's largest,
which changes no bit of the result.  What per-frame factor a row carries cancels in g / (y * Z) (ctc_fast.pyx:138-145).

The reference divides each row by its band sum and multiplies the two normalised rows: where the forward and backward
normalisers have drifted apart, the overlap sum_s alpha_t[s] beta_t[s] of ITS rows is a denormal or 0 and its gradient
there is rounding noise or y itself.  `reference_overlap` restates that number per frame, from the reference's own
recursion, so that a test can tell the frames where the reference is sound from the others.

The two forms differ where a row spans more than float64's range.  At T = 8000 / U = 800 on flat random probabilities
(tests/test_ctc_store_model.inputs(8000, 800, 33, 12)) it does: the paths that advance slowly -- the ones that carry the
likelihood in the end -- fall more than 2^1074 behind each row's largest element on the way and are flushed, in the
reference, in "row" and in every kernel alike: the reference's cost there is 25392.863 where the likelihood's is
25186.541, and its gradient is the gradient of the paths that survived.  "row" is therefore what a kernel with the
reference's rows can be held to; "element" says how far all of them are from the truth.
"""
import numpy as np

from tests import test_ctc_store_model as store_model

LN2 = float(np.log(2.0))
NEG = -(1 << 30)      # exponent of a zero


def _rows(y, seq, blank, per_element, allow_repeats=False):
    """alpha as mantissas [T][L] (0 or in [0.5, 1)) and binary exponents [T][L] (int32; NEG for a zero), labels [L]"""
    A, T = y.shape
    U = len(seq)
    L = 2 * U + 1
    lab = np.full(L, blank, dtype=np.int64)
    lab[1::2] = seq
    allow = np.zeros(L, bool)
    for s in range(3, L, 2):
        allow[s] = allow_repeats or seq[(s - 1) // 2] != seq[(s - 1) // 2 - 1]
    M = np.zeros((T, L))
    E = np.full((T, L), NEG, dtype=np.int32)
    n = np.zeros(L)
    n[0], n[1] = y[blank, 0], y[seq[0], 0]
    z1, zn = np.zeros(1), np.full(1, NEG, dtype=np.int64)
    e_row = 0
    for t in range(T):
        if not per_element:
            if t:
                p = n
                n = p.copy()
                n[1:] += p[:-1]
                n[2:] += np.where(allow[2:], p[:-2], 0.0)
                n *= y[lab, t]
                n[:max(0, L - 2 * (T - t))] = 0                              # ctc_fast.pyx:49-53
            top = n.max()
            if top > 0:
                e = int(np.frexp(top)[1])
                n = np.ldexp(n, -e)                                          # exact but for the flush 2^1074 below `top`
                e_row += e
            m, e = np.frexp(n)
            M[t], E[t] = m, np.where(m != 0, e + e_row, NEG)
            continue
        if t == 0:
            m, e = np.frexp(n)
            e = np.where(m != 0, e, NEG).astype(np.int64)
        else:
            m1, e1 = np.concatenate([z1, m[:-1]]), np.concatenate([zn, e[:-1]])
            m2 = np.concatenate([z1, z1, m[:-2]])
            e2 = np.concatenate([zn, zn, e[:-2]])
            m2, e2 = np.where(allow, m2, 0.0), np.where(allow, e2, NEG)
            top = np.maximum(np.maximum(e, e1), e2)
            # the three terms on the largest one's exponent: a term 2^-1100 below it changes no bit of the sum
            tot = (np.ldexp(m, np.maximum(e - top, -1100)) + np.ldexp(m1, np.maximum(e1 - top, -1100))
                   + np.ldexp(m2, np.maximum(e2 - top, -1100)))
            tot = tot * y[lab, t]                                            # in [0.5, 3) * y: no underflow
            tot[:max(0, L - 2 * (T - t))] = 0                                # ctc_fast.pyx:49-53
            m, de = np.frexp(tot)
            e = np.where(m != 0, top + de, NEG)
        M[t], E[t] = m, e
    return M, E, lab


def _row_sum(m, e):
    """(sum, exponent) of rows given as mantissas and exponents: sum * 2^exponent, sum in [0.5, L)"""
    top = e.max(axis=-1, keepdims=True).astype(np.int64)
    return np.ldexp(m, np.maximum(e - top, -1100)).sum(axis=-1), top[..., 0]


def reference_overlap(y, seq, blank=0):
    """[T]: sum_s alpha_t[s] * beta_t[s] of the reference's sum-normalised float64 rows, formed its way"""
    y = np.asarray(y, dtype=np.float64)
    seq = np.asarray(seq)
    with np.errstate(all="ignore"):
        al, _ = store_model.lattice(y, seq, blank)
        be_r, _ = store_model.lattice(np.asfortranarray(y[:, ::-1]), seq[::-1].copy(), blank)
        return (al * be_r[::-1, ::-1]).sum(axis=1)


def exact(y, seq, blank=0, rows="element", mutate=None, overlap_log2=False):
    """y: float64 (A, T); seq: int labels.  Returns (cost, grad (A, T), skip): what ctc_fast.ctc_loss returns, without
    the underflow of its forward-backward product (rows="row") or without any underflow (rows="element").
    mutate (tests only): "drop_exponent" forgets beta's exponent in the product; "allow_repeats" takes the skip
    transition between equal labels too; "per_label" sums Z = sum_k g[k] / y[k] over the labels instead of over the
    states (the same sum in exact arithmetic).  overlap_log2: a fourth value, [T]: log2 of sum_s alpha_t[s] beta_t[s] with both
    rows scaled so that their largest element is in [0.5, 1) (-inf where no state has both) -- the magnitude a kernel's
    product of two rescaled rows has, whether or not float64 can hold it."""
    assert rows in ("row", "element")
    y = np.asarray(y, dtype=np.float64)
    seq = np.asarray(seq)
    A, T = y.shape
    ma, ea, lab = _rows(y, seq, blank, rows == "element", mutate == "allow_repeats")
    mb, eb, _ = _rows(np.ascontiguousarray(y[:, ::-1]), seq[::-1].copy(), blank, rows == "element", mutate == "allow_repeats")
    mb, eb = mb[::-1, ::-1], eb[::-1, ::-1]
    sa, xa = _row_sum(ma, ea)
    dead = np.nonzero(sa == 0)[0]
    if dead.size and not (2 * len(seq) + 1 >= 2 * T + 2 and T > 1):
        # a zero band sum: the reference's except-branch (ctc_fast.pyx:147-149): -llForward as far as alpha got
        t0 = int(dead[0])
        cost = -(float(xa[t0 - 1]) * LN2 + float(np.log(sa[t0 - 1]))) if t0 else 0.0
        return cost, np.zeros_like(y), True
    with np.errstate(divide="ignore"):
        cost = -(float(xa[T - 1]) * LN2 + float(np.log(sa[T - 1])))         # empty band: log(0) -> +inf like :70-76
    # ---- products with the exponents combined first
    live = (ma != 0) & (mb != 0)
    es = np.where(live, ea.astype(np.int64) + (0 if mutate == "drop_exponent" else eb), NEG)
    emax = es.max(axis=1, keepdims=True)
    ab = np.where(live, np.ldexp(ma * mb, np.maximum(es - emax, -1100)), 0.0)   # a frame's largest is in [0.25, 1)
    ylab = y[lab, :].T
    g = np.zeros_like(y)
    for k in range(A):
        sel = lab == k
        if sel.any():
            g[k] = ab[:, sel].sum(axis=1)
    with np.errstate(all="ignore"):
        if mutate == "per_label":
            Z = np.where(g != 0, g / np.where(y == 0, 1, y), 0.0).sum(axis=0)
        else:
            Z = np.where(ab != 0, ab / np.where(ylab == 0, 1, ylab), 0.0).sum(axis=1)      # :125-136
    tmp = y * Z
    grad = np.where(tmp > 0, y - g / np.where(tmp > 0, tmp, 1), y)          # :138-145
    if not overlap_log2:
        return cost, grad, False
    with np.errstate(divide="ignore"):
        mag = np.where(live.any(axis=1), emax[:, 0] - ea.max(axis=1).astype(np.int64) - eb.max(axis=1), 0) + np.log2(ab.sum(axis=1))
    return cost, grad, False, mag
