"""Python restatement of the prefix beam search of DESIGN.md §4.5 (the reference's
``BeamLMDecoder.decode``, ctc_fast/new_decoder/decoder.pyx:136-193), written the way the
device kernel works: float32 beam state between frames, float64 accumulation, the
max-shifted combine, candidates ordered by (key descending, cell index ascending) with cell
index = beam rank * A + symbol (0 = the prefix itself).  The yardstick of the GPU tests."""
import math

import numpy as np

NEG = float("-inf")


def lse(*xs):
    m = max(xs)
    if m == NEG:
        return NEG
    return m + math.log(sum(math.exp(x - m) for x in xs))


def f32(x):
    return float(np.float32(x))


def decode(probs, beam=40, alpha=1.0, beta=0.0, lm_row=None, nbest=1):
    """probs: (A, T) natural-log probabilities.  lm_row(prefix tuple) -> A log10 values
    (None: no LM term).  Returns [(prefix tuple, score)] of the best ``nbest``."""
    probs = np.asarray(probs, dtype=np.float64)
    A, T = probs.shape
    # beam: list of (prefix, p_nb f32, p_b f32, key f64), best first
    cur = [((), NEG, 0.0, 0.0)]
    hold = {}                      # previous frame's candidates: prefix -> (p_nb f32, p_b f32)
    rows = {(): np.asarray(lm_row(()), dtype=np.float32)} if lm_row is not None else {}
    for t in range(T):
        y = probs[:, t]
        idx = {p: j for j, (p, _, _, _) in enumerate(cur)}
        cells = []                 # (key, cell index, prefix, nb, b)
        for j, (P, v0, v1, _) in enumerate(cur):
            l = P[-1] if P else -1
            nb = [v0 + y[l]] if P else []
            if P and P[:-1] in idx:
                pj = idx[P[:-1]]
                _, w0, w1, _ = cur[pj]
                lm = alpha * rows[P[:-1]][l] if lm_row is not None else 0.0
                if len(P) == 1 or P[-2] != l:
                    nb.append(w0 + y[l] + lm)
                nb.append(w1 + y[l] + lm)
            nbv = lse(*nb) if nb else NEG
            bv = lse(v0 + y[0], v1 + y[0])
            cells.append((lse(nbv, bv) + beta * len(P), j * A, P, nbv, bv))
            for c in range(1, A):
                Q = P + (c,)
                if Q in idx:
                    continue
                lm = alpha * rows[P][c] if lm_row is not None else 0.0
                nb = [v1 + y[c] + lm]
                if c != l:
                    nb.append(v0 + y[c] + lm)
                h2, h3 = hold.get(Q, (NEG, NEG))
                nb.append(h2 + y[c])
                nbv = lse(*nb)
                bv = lse(h2 + y[0], h3 + y[0])
                cells.append((lse(nbv, bv) + beta * len(Q), j * A + c, Q, nbv, bv))
        hold = {P: (f32(nbv), f32(bv)) for _, _, P, nbv, bv in cells}
        cells.sort(key=lambda e: (-e[0], e[1]))
        cur = [(P, f32(nbv), f32(bv), key) for key, _, P, nbv, bv in cells[:beam]]
        if lm_row is not None:
            rows = {P: (rows[P] if P in rows else np.asarray(lm_row(P), dtype=np.float32))
                    for P, _, _, _ in cur}
    return [(P, key) for P, _, _, key in cur[:nbest]]


def arpa_rows(lm, sym_words):
    """lm_row for decode(): P -> float32 log10 P(symbol | <s> + P) for every symbol"""
    A = len(sym_words)

    def row(P):
        ctx = [lm.bos] + [int(sym_words[s]) for s in P]
        out = np.zeros(A, dtype=np.float32)
        for c in range(1, A):
            out[c] = lm.score_ids(ctx, int(sym_words[c]))
        return out
    return row
