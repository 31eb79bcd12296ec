"""Python restatement of the prefix beam search of DESIGN.md §4.5 (the reference's
``BeamLMDecoder.decode``, ctc_fast/new_decoder/decoder.pyx:136-193), written the way the
device kernel works: float32 beam state between frames, float64 accumulation, the
max-shifted combine, candidates ordered by (key descending, cell index ascending) with cell
index = beam rank * A + symbol (0 = the prefix itself).  The yardstick of the GPU tests.

alpha * LM is a float64 product, as in the reference (Python floats) and in the kernel
(``p.alpha * (double)row``): ``alpha * row[c]`` with a NumPy float32 scalar would be multiplied
and rounded in float32 (NumPy 2 keeps the array scalar's type), invisible only while alpha is
a float32 number."""
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


BEAM_CELL, EXT_CELL = 0, 1         # trace "kinds": the cell of a beam entry / of an extension


def decode(probs, beam=40, alpha=1.0, beta=0.0, lm_row=None, nbest=1, trace=None):
    """probs: (A, T) natural-log probabilities.  lm_row(prefix tuple) -> A log10 values
    (None: no LM term).  Returns [(prefix tuple, score)] of the best ``nbest``.

    trace: a list that receives one dict per frame: ``beam`` the whole new beam in rank order
    as (prefix, key); ``kinds`` the kind of cell each entry came from (BEAM_CELL: the prefix
    was a beam entry, EXT_CELL: an extension; the two sum their terms in different orders);
    ``cut`` / ``cut_kind`` / ``cut_prefix`` the key, kind and prefix of the best candidate that
    was not kept (None when every candidate was kept)."""
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
                lm = alpha * float(rows[P[:-1]][l]) if lm_row is not None else 0.0
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
                lm = alpha * float(rows[P][c]) if lm_row is not None else 0.0
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
        if trace is not None:
            kind = lambda e: BEAM_CELL if e[1] % A == 0 else EXT_CELL
            cut = cells[beam] if len(cells) > beam else None
            trace.append({"beam": [(e[2], e[0]) for e in cells[:beam]],
                          "kinds": [kind(e) for e in cells[:beam]],
                          "cut": cut[0] if cut else None,
                          "cut_kind": kind(cut) if cut else None,
                          "cut_prefix": cut[2] if cut else None})
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
