"""Whole-beam comparison of the prefix beam search kernel with tests/beam_model.py, frame by
frame: the inputs, the preconditions that are asserted on the model alone, and
the rules by which a decoded truncation batch is compared with the model's trace.

The beam after frame t of an utterance is the final beam of its truncation lp[:, :t], so one
``decode_beam_batch([lp[:, :t] for t in 1..T], nbest=beam)`` call returns every rank of every
frame.  Everything here follows from the suite's key tolerance tol(k) = 1e-6 |k| + 1e-9:

* two neighbours of the model's beam are *separated* when their keys differ by more than
  tol(k_i) + tol(k_j) (each may move by its tol); separated neighbours must come in the model's
  order, a run of non-separated neighbours is compared as a set of prefixes;
* ``-inf`` keys are exact on any hardware: a finite key next to ``-inf`` is separated, and a run
  of ``-inf`` keys has to come in the model's order (ascending cell index).  The cell index hangs
  on the ranks of the parents, so the model must show no non-separated pair in any earlier frame;
* with ``exact_ties`` (inputs built to tie), finite neighbours with bit-equal keys that come from
  cells of one kind are an exact tie as well and have to come in the model's order; equal keys
  from cells of different kinds sum their terms in different orders, where libm and the device
  need not agree to the bit, so the model must not rely on them;
* membership at the cut is defined when the model's last kept key exceeds the best cut key by
  more than the two tols, or when both are ``-inf`` / an exact tie of one kind.
"""
import numpy as np

from tests import beam_model

NEG = float("-inf")


def tol(k):
    return 1e-6 * abs(k) + 1e-9


def logsoftmax(x):
    m = x.max(axis=0, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))


def peaked(rs, A, T, sharp=6.0):
    """the generator of tests/test_gpu_decode.py: a random path of runs over noise"""
    x = 1.5 * rs.randn(A, T)
    t = 0
    while t < T:
        s = rs.randint(1, A) if rs.rand() < 0.6 else 0
        r = rs.randint(1, 4)
        x[s, t:t + r] += sharp
        t += r
    return logsoftmax(x)


def sparse_frames(rs, A, T):
    """one finite symbol per frame, two on every sixth frame: almost every candidate is -inf"""
    lp = np.full((A, T), NEG)
    for t in range(T):
        k = 2 if t % 6 == 5 else 1
        syms = rs.choice(A, size=k, replace=False)
        lp[syms, t] = np.log(rs.rand(k) * 0.5 + 0.25)
    return lp


def dead_frame(rs, A, T, dead):
    """dense frames and one frame where nothing is possible: every key after it is -inf"""
    lp = logsoftmax(2.0 * rs.randn(A, T))
    lp[:, dead] = NEG
    return lp


def twins(rs, A, T, pairs):
    """peaked posteriors in which the symbols of each pair have identical columns"""
    x = 1.5 * rs.randn(A, T)
    t = 0
    while t < T:
        s = rs.randint(1, A) if rs.rand() < 0.6 else 0
        r = rs.randint(1, 4)
        x[s, t:t + r] += 3.0
        t += r
    for a, b in pairs:
        x[b] = x[a]
    return logsoftmax(x)


def model_trace(lp, beam, alpha, beta, rows):
    tr = []
    beam_model.decode(lp, beam, alpha, beta, rows, trace=tr)
    return tr


def pair_rule(ka, kb, kind_a, kind_b, exact_ties):
    """'sep' (separated), 'tie' (exact, the model's order is demanded), 'near' (compared as a
    set) or 'mixed' (bit-equal keys from cells of different kinds) for two neighbours ka >= kb"""
    if ka == NEG and kb == NEG:
        return "tie"
    if kb == NEG:
        return "sep"
    if ka - kb > tol(ka) + tol(kb):
        return "sep"
    if exact_ties and ka == kb:
        return "tie" if kind_a == kind_b else "mixed"
    return "near"


def check_model(trace, beam, exact_ties=False, near_cap=0.02):
    """The preconditions, asserted on the model's trace alone.  Returns counts: neighbour pairs,
    non-separated ('near') pairs, exact finite ties, frames whose cut falls inside a -inf tie
    and inside an exact finite tie."""
    st = dict(pairs=0, near=0, ties=0, inf_ties=0, cut_in_inf_tie=0, cut_in_tie=0, frames=len(trace))
    near_before = 0
    for t, fr in enumerate(trace):
        keys = [k for _, k in fr["beam"]]
        kinds = fr["kinds"]
        assert len(keys) <= beam and (fr["cut"] is None or len(keys) == beam)
        if keys[-1] == NEG and (fr["cut"] == NEG or (len(keys) > 1 and keys[-2] == NEG)):
            assert near_before == 0, ("frame %d orders -inf cells after a non-separated pair" % t)
        assert len({P for P, _ in fr["beam"]}) == len(keys), "a prefix twice in the model's beam"
        for i in range(len(keys) - 1):
            assert keys[i] >= keys[i + 1]
            r = pair_rule(keys[i], keys[i + 1], kinds[i], kinds[i + 1], exact_ties)
            assert r != "mixed", ("frame %d ranks %d/%d tie across cell kinds" % (t, i, i + 1))
            if exact_ties:
                assert r != "near", ("frame %d ranks %d/%d closer than 2 tol, not equal" % (t, i, i + 1))
            st["pairs"] += 1
            st["near"] += r == "near"
            if r == "tie":
                st["inf_ties" if keys[i] == NEG else "ties"] += 1
        if fr["cut"] is not None:
            r = pair_rule(keys[-1], fr["cut"], kinds[-1], fr["cut_kind"], exact_ties)
            gap = keys[-1] - fr["cut"] if keys[-1] != NEG else 0.0
            assert r in ("sep", "tie"), ("frame %d: the cut is not defined: last kept %r, best cut %r (%s)"
                                         % (t, keys[-1], fr["cut"], r), gap)
            if r == "tie":
                st["cut_in_inf_tie" if keys[-1] == NEG else "cut_in_tie"] += 1
        near_before = st["near"]
    assert st["near"] <= near_cap * max(1, st["pairs"]), st
    return st


def truncations(lp):
    return [lp[:, :t] for t in range(1, lp.shape[1] + 1)]


def compare(trace, hyps, scores, beam, exact_ties=False, what=""):
    """hyps / scores: decode_beam_batch(truncations(lp), nbest=beam).  Returns the largest
    |got - model| / |model| over the finite keys."""
    worst = 0.0
    assert len(hyps) == len(trace) and scores.shape == (len(trace), beam)
    for t, fr in enumerate(trace):
        model = fr["beam"]
        n = len(model)
        got_p = [tuple(int(s) for s in h) for h in hyps[t]]
        got_k = [float(s) for s in scores[t]]
        # beyond the beam: empty hypotheses, -inf scores
        for r in range(n, beam):
            assert got_k[r] == NEG and got_p[r] == (), (what, t, r, got_k[r], got_p[r])
        for r, (P, k) in enumerate(model):
            if k == NEG:
                assert got_k[r] == NEG, (what, t, r, got_k[r])
            else:
                assert abs(got_k[r] - k) <= tol(k), (what, t, r, got_k[r], k)
                if k != 0.0:
                    worst = max(worst, abs(got_k[r] - k) / abs(k))
        r = 0
        while r < n:
            e = r
            while e + 1 < n and pair_rule(model[e][1], model[e + 1][1], fr["kinds"][e], fr["kinds"][e + 1],
                                          exact_ties) == "near":
                e += 1
            want = [P for P, _ in model[r:e + 1]]
            got = got_p[r:e + 1]
            if e == r:
                assert got == want, (what, "frame", t, "rank", r, got, want, model[r][1])
            else:
                assert sorted(got) == sorted(want), (what, "frame", t, "ranks", r, e, got, want)
            r = e + 1
    return worst


# ---- LM rows read off the decoder's output ---------------------------------------------------

def forced_prefix_frames(rs, A, P):
    """frames s1, blank, s2, blank, ..., sn, blank with one finite symbol each, then one frame with
    every symbol finite.  With beta = 0, beam >= A + 1 and nbest = beam the final beam holds P and
    every P+c, each with a single-term sum (p_nb of P is -inf after a blank frame), so
    key(P+c) - key(P) = y[c] - y[0] + alpha * lm(c | <s> P) exactly."""
    T = 2 * len(P) + 1
    lp = np.full((A, T), NEG)
    for i, s in enumerate(P):
        lp[s, 2 * i] = np.log(rs.rand() * 0.6 + 0.3)
        lp[0, 2 * i + 1] = np.log(rs.rand() * 0.6 + 0.3)
    lp[:, T - 1] = logsoftmax(rs.randn(A, 1))[:, 0]
    return lp


def lm_row_prefixes(lm, sw, rs, per_order=5):
    """forced prefixes for a row check: walks ``lm.ngrams`` so that the longest match stops at every
    possible n, random leads so that longer contexts are missing and the back-off chain breaks,
    every length 0 .. order + 2 (the context truncation), the symbols mapped to <unk>, a repeated
    symbol."""
    A = len(sw)
    inv = {}
    for s in range(1, A):
        inv.setdefault(int(sw[s]), []).append(s)
    unk_syms = inv[lm.unk]
    assert 4 in unk_syms and len(unk_syms) >= 2
    known = [s for s in range(1, A) if s not in unk_syms]
    out = [(), (unk_syms[0],), (known[0], unk_syms[-1]), (unk_syms[-1], known[1], known[2]),
           (known[3], known[3]), (known[4], known[4], known[4], known[5])]
    by_len = {}
    for g in lm.ngrams:
        body = g[1:] if g[0] == lm.bos else g
        if all(w in inv for w in body):
            by_len.setdefault(len(g), []).append(g)
    for m in sorted(by_len):
        gs = sorted(by_len[m])
        for i in rs.permutation(len(gs))[:per_order]:
            g = gs[i]
            syms = tuple(inv[w][rs.randint(len(inv[w]))] for w in (g[1:] if g[0] == lm.bos else g))
            lead = () if g[0] == lm.bos else tuple(int(s) for s in rs.randint(1, A, size=rs.randint(0, 3)))
            out.append((lead + syms)[-(lm.order + 2):] if g[0] != lm.bos else syms)
    for n in range(lm.order + 3):
        out.append(tuple(int(s) for s in rs.randint(1, A, size=n)))
        out.append(tuple(int(s) for s in rs.choice(known[:6], size=n)))
    return sorted(set(out))


def recover_lm_row(P, lp, hyps, keys, alpha):
    """{c: (log10 P(c | <s> P) read off the final beam, |larger of the two keys|)}"""
    at = {tuple(int(s) for s in h): float(k) for h, k in zip(hyps, keys) if k != NEG}
    y = lp[:, -1]
    assert P in at, ("the forced prefix is not in the final beam", P)
    row = {}
    for c in range(1, lp.shape[0]):
        assert P + (c,) in at, ("an extension of the forced prefix is not in the final beam", P, c)
        row[c] = (((at[P + (c,)] - at[P]) - (y[c] - y[0])) / alpha, max(abs(at[P + (c,)]), abs(at[P])))
    return row


def check_lm_rows(lm, sw, prefixes, rows, alpha, what=""):
    """rows[i]: recover_lm_row of prefixes[i], against the textbook back-off in float64.  Per
    value: the scorer adds n float32 terms, each addition rounding by at most 2^-24 of the partial
    sum, and the read-off divides a float64 difference of keys by alpha.  A value with a single term
    is a float32 table entry that went through no float32 addition at all: there only the read-off
    error is allowed, which is what shows an alpha (or an alpha * LM product) carried in float32 --
    its error of up to 2^-24 |lm| hides inside the summation bound everywhere else."""
    from tests.helpers import arpa_backoff, arpa_backoff_terms
    stats = dict(pairs=0, match=set(), early_break=0, full_chain=0, single=0, worst=0.0, worst_single=0.0)
    for P, row in zip(prefixes, rows):
        ctx = [lm.bos] + [int(sw[s]) for s in P]
        for c, (got, kmag) in row.items():
            w = int(sw[c])
            want = arpa_backoff(lm, ctx, w)
            n, terms = arpa_backoff_terms(lm, ctx, w)
            partial = np.abs(np.cumsum(terms)).max()
            bound = len(terms) * 2.0 ** -24 * partial + 1e-12 * kmag / alpha
            assert abs(got - want) <= bound, (what, P, c, got, want, bound, terms)
            if len(terms) == 1:
                assert abs(got - want) <= 1e-12 * kmag / alpha, (what, P, c, got, want, "single term")
                stats["single"] += 1
                stats["worst_single"] = max(stats["worst_single"], abs(got - want) / abs(want))
            stats["worst"] = max(stats["worst"], abs(got - want) / bound)
            longer = min(len(ctx), lm.order - 1) - (n - 1)       # contexts longer than the match
            stats["pairs"] += 1
            stats["match"].add(n)
            stats["early_break"] += len(terms) - 1 < longer
            stats["full_chain"] += longer > 0 and len(terms) - 1 == longer
    return stats
