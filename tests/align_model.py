"""The contract of the CTC forced alignment (include/sctc.h) in NumPy, vectorised over
the states of the extended row, and a brute-force enumerator for tiny shapes.

Input: natural-log probabilities ``y`` of one utterance as an (A, T) array (float32 is widened exactly
to float64), a label row ``l[0..U)`` and the blank.  Extended row x[s], s = 0..2U (S = 2U+1):
x[2u+1] = l[u], even s the blank (ctc_fast.pyx:42-76).

    v_0(0) = y_0(blank), v_0(1) = y_0(x[1]), the other states -inf
    v_t(s) = best(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s odd and x[s] != x[s-2]) + y_t(x[s])

``best`` takes the largest value, on ties the first of (stay, s-1, s-2); all candidates -inf gives -inf
with back-pointer "stay".  The path ends in state S-1 unless v_{T-1}(S-2) is strictly larger.  The
Viterbi score is that end value: a plain chain of float64 additions, so an implementation is bit-equal.
The total replaces ``best`` by the max-shifted log-sum-exp (-inf (+) -inf = -inf) and is
a_{T-1}(S-1) (+) a_{T-1}(S-2) = log P_ctc(l | y).

status 0: aligned.  1: no alignment of finite score (scores -inf, every frame_label and span -1).
2: a label outside [0, A) or equal to the blank (outputs as for 1).  T = 0: status 0 with scores 0.0
when U = 0, else status 1.  Without ``total`` the total is NaN.
"""
import itertools

import numpy as np

NINF = -np.inf


def _lse(*xs):
    """max-shifted log-sum-exp of arrays, -inf where every term is -inf"""
    with np.errstate(all="ignore"):
        m = xs[0]
        for x in xs[1:]:
            m = np.maximum(m, x)
        safe = np.where(np.isfinite(m), m, 0.0)
        acc = np.zeros_like(safe)
        for x in xs:
            acc = acc + np.exp(x - safe)
        return np.where(m == NINF, NINF, safe + np.log(np.where(acc > 0, acc, 1.0)))


class Alignment(object):
    __slots__ = ("frame_label", "span", "viterbi", "total", "status")

    def __init__(self, frame_label, span, viterbi, total, status):
        self.frame_label, self.span, self.viterbi, self.total, self.status = frame_label, span, viterbi, total, status


def _failed(T, U, status, total):
    return Alignment(np.full(T, -1, np.int32), np.full((U, 2), -1, np.int32), NINF, NINF if total else np.nan, status)


def align(y, labels, blank=0, total=False):
    """the contract for one utterance; y (A, T), labels int sequence -> Alignment"""
    y = np.asarray(y)
    A, T = y.shape
    y = y.astype(np.float64)
    l = np.asarray(labels, dtype=np.int64).reshape(-1)
    U = l.shape[0]
    S = 2 * U + 1
    if U and (l.min() < 0 or l.max() >= A or np.any(l == blank)):
        return _failed(T, U, 2, total)
    if T == 0:
        if U == 0:
            return Alignment(np.zeros(0, np.int32), np.zeros((0, 2), np.int32), 0.0, 0.0 if total else np.nan, 0)
        return _failed(T, U, 1, total)
    x = np.full(S, blank, dtype=np.int64)
    x[1::2] = l
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = l[1:] != l[:-1]
    with np.errstate(all="ignore"):
        v = np.full(S, NINF)
        v[0] = y[blank, 0]
        if S > 1:
            v[1] = y[x[1], 0]
        a = v.copy()
        bp = np.zeros((T, S), dtype=np.int8)
        pad = np.full(2, NINF)
        for t in range(1, T):
            ext = np.concatenate([pad, v])
            c0, c1 = ext[2:], ext[1:-1]
            c2 = np.where(skip, ext[:-2], NINF)
            m = c0.copy()
            q = np.zeros(S, dtype=np.int8)
            w = c1 > m
            m[w] = c1[w]
            q[w] = 1
            w = c2 > m
            m[w] = c2[w]
            q[w] = 2
            yt = y[x, t]
            v = m + yt
            bp[t] = q
            if total:
                ea = np.concatenate([pad, a])
                a = _lse(ea[2:], ea[1:-1], np.where(skip, ea[:-2], NINF)) + yt
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    vit = float(v[s])
    if not vit > NINF:
        return _failed(T, U, 1, total)
    tot = np.nan
    if total:
        tot = float(_lse(a[S - 1:S], a[S - 2:S - 1] if S >= 2 else np.full(1, NINF))[0])
    states = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s]) if t > 0 else 0
    fl = np.where(states & 1, (states - 1) >> 1, -1).astype(np.int32)
    span = np.full((U, 2), -1, np.int32)
    for u in range(U):
        fr = np.nonzero(fl == u)[0]
        span[u] = (fr[0], fr[-1])
    return Alignment(fl, span, vit, tot, 0)


def align_batch(ys, seqs, blank=0, total=False):
    """the model of ctc_fast.align_batch: (frame_label list, span list, viterbi, total or None, status)"""
    res = [align(y, s, blank, total) for y, s in zip(ys, seqs)]
    return ([r.frame_label for r in res], [r.span for r in res], np.array([r.viterbi for r in res], np.float64),
            np.array([r.total for r in res], np.float64) if total else None, np.array([r.status for r in res], np.int32))


def collapse(path, blank=0):
    """the CTC collapse of a frame-level symbol path: merge repeats, drop blanks"""
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def enumerate_paths(y, labels, blank=0):
    """(viterbi, total) of the label row by enumeration of all A^T frame-level paths: the largest sum and
    the log of the summed probabilities of the paths that collapse to it; (-inf, -inf) when there is none"""
    y = np.asarray(y, dtype=np.float64)
    A, T = y.shape
    want = [int(c) for c in labels]
    best, scores = NINF, []
    with np.errstate(all="ignore"):
        for path in itertools.product(range(A), repeat=T):
            if collapse(path, blank) != want:
                continue
            sc = 0.0
            for t, c in enumerate(path):
                sc += y[c, t]
            scores.append(sc)
            best = max(best, sc)
        if not scores or best == NINF:
            return NINF, NINF
        sc = np.array(scores)
        return float(best), float(best + np.log(np.exp(sc - best).sum()))
