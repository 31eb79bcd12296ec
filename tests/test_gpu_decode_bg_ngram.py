"""GPU checks of the lexicon-constrained beam search with a word n-gram LM of order 2..5
(csrc/ctc_beam.hip ``ctc_lexngbeam_kernel``) through the public Python and C surfaces:
the Python restatement (tests/lex_ngram_beam_model.py, with a brute-force LM on the ARPA text) with
``nbest = beam``, bit-equality with the word-bigram kernel at order 2, LM terms read off forced paths,
the lexicon property of every returned hypothesis in the ABI's corners, and runDecode.py --method bg
--word-lm-order 4."""
import pickle

import numpy as np
import pytest

from tests import lex_ngram_beam_model as ngm
from tests.beam_harness import PATTERN, raw_decode
from tests.beam_trace import logsoftmax, tol
from tests.test_dataloader import write_shard
from tests.test_decode_bg_cpu import CHARS, WORDS, fixture_lexicon
from tests.test_gpu_decode_bg import SPACE, check_lexicon_property
from tests.test_lexicon_ngram_cpu import ARPA4, filtered_bigram_file

pytestmark = pytest.mark.gpu

NEG = float("-inf")
A = 35
ALPHA, BETA = 0.8, 0.37

_CACHE = {}


def chars_words():
    from decoder import decoder_utils
    if "cw" not in _CACHE:
        _CACHE["cw"] = (decoder_utils.load_chars(CHARS), decoder_utils.load_words(WORDS))
    return _CACHE["cw"]


def brute(order):
    if ("brute", order) not in _CACHE:
        _CACHE[("brute", order)] = ngm.BruteLM(ARPA4, order)
    return _CACHE[("brute", order)]


def device_lexicon(order, size="large"):
    """(DecodeLexicon of the fixture lexicon with the 4-gram file read at ``order``, child, word)"""
    import ctc_fast
    if ("lex", order, size) not in _CACHE:
        chars, words = chars_words()
        lex, sp = fixture_lexicon(words, A, size)
        d = ctc_fast.DecodeLexicon(lex, chars, ARPA4, "[space]", specials=sp, A=A, order=order)
        assert d.order == order and (order == 2 or d.lm.order == order)     # order 2 with a path: decoder.lm.LM
        _CACHE[("lex", order, size)] = (d,) + tuple(d.tree.flatten(A))
    return _CACHE[("lex", order, size)]


def model_top(lp, order, beam, nbest, size="large", alpha=ALPHA, beta=BETA):
    d, child, word = device_lexicon(order, size)
    return ngm.decode(lp, child, word, brute(order).prob_ids, d.lm.start, SPACE, order, beam=beam, alpha=alpha,
                      beta=beta, nbest=nbest)


def spell(chars, w):
    return [chars[w]] if w.startswith("[") else [chars[ch] for ch in w]


def lm_word_path(rs, T, blank_p=0.25):
    """frame labels of a word sequence that follows the listed n-grams three times out of four, so that
    the search meets trigrams and 4-grams and not only back-offs"""
    chars, words = chars_words()
    b = brute(4)
    if "follow" not in _CACHE:
        ok = set(words) | {"[noise]", "[laughter]"}
        follow = {}
        for g in b.grams:
            if len(g) >= 2 and g[-1] in ok:
                follow.setdefault(g[:-1], []).append(g[-1])
        _CACHE["follow"] = {k: sorted(v) for k, v in follow.items()}
    follow = _CACHE["follow"]
    hist, path = ["<s>"], []
    while len(path) < T:
        nxt = follow.get(tuple(hist[-rs.randint(1, 4):]))
        w = nxt[rs.randint(len(nxt))] if nxt and rs.rand() < 0.75 else words[rs.randint(len(words))]
        hist.append(w if (w,) in b.grams else "<UNK>")
        for s in spell(chars, w) + [SPACE]:
            if (path and path[-1] == s) or rs.rand() < blank_p:
                path += [0] * rs.randint(1, 3)
            path += [s] * rs.randint(1, 4)
    return np.array(path[:T])


def posteriors(rs, T, kind="peaked", sharp=6.0):
    if kind == "flat":
        return logsoftmax(0.4 * rs.randn(A, T))
    x = 1.5 * rs.randn(A, T)
    path = lm_word_path(rs, T)
    x[path, np.arange(T)] += sharp
    lp = logsoftmax(x)
    if kind == "neginf":
        mask = rs.rand(A, T) < 0.15
        mask[path, np.arange(T)] = False
        mask[0, :] = False
        lp[mask] = NEG
    return lp


# ---- 1. the restatement --------------------------------------------------------------------------

RESTATEMENT = [(order, T, beam, "peaked") for order in (3, 4) for T in (60, 300) for beam in (16, 40, 64)]
RESTATEMENT += [(4, 60, 40, "flat"), (3, 60, 40, "neginf")]


def restatement_input(order, T, beam, kind):
    """the seeds were tried on the model alone: every case leaves at most 5 % of its hypotheses
    uncompared (asserted below before the device is asked)"""
    return posteriors(np.random.RandomState(1000 * order + T + beam), T, kind)


def clear_ranks(keys):
    """ranks whose neighbours are further away than the two tolerances"""
    n = len(keys)
    return [i for i in range(n)
            if all(abs(keys[i] - keys[m]) > tol(keys[i]) + tol(keys[m]) for m in (i - 1, i + 1) if 0 <= m < n)]


@pytest.mark.parametrize("order,T,beam,kind", RESTATEMENT)
def test_against_restatement(order, T, beam, kind):
    import ctc_fast
    d, child, word = device_lexicon(order)
    assert word.shape[0] > 700 and (word >= 0).sum() == 363
    lp = restatement_input(order, T, beam, kind)
    top = model_top(lp, order, beam, beam)
    assert len(top) == beam
    keys = [k for _, k in top]
    clear = clear_ranks(keys)
    assert beam - len(clear) <= 0.05 * beam, "near ties in the model itself: pick another seed"
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=d, beam=beam, alpha=ALPHA, beta=BETA, nbest=beam)
    worst = max(abs(scores[0, n] - keys[n]) / tol(keys[n]) for n in range(beam))
    print("order %d T %d beam %d %s: worst key difference %.3g of the tolerance, %d of %d hypotheses compared"
          % (order, T, beam, kind, worst, len(clear), beam))
    for n in range(beam):
        assert abs(scores[0, n] - keys[n]) <= tol(keys[n]), (n, scores[0, n], keys[n])
        check_lexicon_property(hyps[0][n], child, word)
    for n in clear:
        assert list(hyps[0][n]) == list(top[n][0]), n
    if kind == "peaked":
        assert list(hyps[0][0]).count(SPACE) >= T // 40


# ---- 2. order 2 is the bigram kernel, bit for bit -------------------------------------------------

@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_order_2_is_bit_equal_to_the_bigram_kernel(dt, tmp_path_factory):
    import ctc_fast
    from decoder import lm as lm_mod, ngram_lm
    path = filtered_bigram_file(tmp_path_factory.getbasetemp())
    chars, words = chars_words()
    lex, sp = fixture_lexicon(words, A, "large")
    if "pair" not in _CACHE:
        _CACHE["pair"] = (ctc_fast.DecodeLexicon(lex, chars, lm_mod.LM(path), "[space]", specials=sp, A=A),
                          ctc_fast.DecodeLexicon(lex, chars, ngram_lm.NgramLM(path, 2), "[space]", specials=sp, A=A))
    old, new = _CACHE["pair"]
    assert old.order == new.order == 2 and isinstance(new.lm, ngram_lm.NgramLM) and isinstance(old.lm, lm_mod.LM)
    T, beam = 200, 40
    from tests.test_gpu_decode_bg import peaked_words
    lp = peaked_words(np.random.RandomState(200), A, T, chars, lex).astype(dt)
    host = np.ascontiguousarray(lp.T)
    out = [raw_decode("lexbeam", host, A, A, [T], [0], beam, beam, h, ALPHA, BETA) for h in (old, new)]
    (h0, s0, l0, _, w0), (h1, s1, l1, _, w1) = out
    assert w0 == w1                                                   # the workspace formula is the same
    assert s0.tobytes() == s1.tobytes() and l0.tobytes() == l1.tobytes()
    assert np.isfinite(s0).all() and l0.min() > 10
    for n in range(beam):
        assert h0[0][n].tobytes() == h1[0][n].tobytes()
    ph, ps = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=new, beam=beam, alpha=ALPHA, beta=BETA, nbest=beam)
    assert ps.tobytes() == s0.tobytes()


# ---- 3. LM terms read off forced paths -----------------------------------------------------------

def forced_cases():
    """{what: (sentence, order, the value the last word must get or None)} from the listed n-grams of the
    fixture; every word is in the lexicon, and in the LM unless the case is about <UNK>"""
    if "forced" in _CACHE:
        return _CACHE["forced"]
    chars, words = chars_words()
    b = brute(4)
    G = b.grams
    ok = (set(words) | {"[noise]", "[laughter]"}) & set(b.ids)
    known = sorted(ok)
    good = lambda g: all(w in ok for w in g)
    tri = sorted(g for g in G if len(g) == 3 and good(g))
    four = sorted(g for g in G if len(g) == 4 and good(g))
    out = {"start": ([known[3]], 4, None)}
    g = next(g for g in tri if g[1:] in G)
    out["listed_trigram"] = (list(g), 3, G[g][0])
    g = next(g for g in four if g[1:] in G and g[2:] in G)
    out["listed_4gram"] = (list(g), 4, G[g][0])
    # five words at order 4: <s> and the first word have left the history when the last word is scored
    out["history_truncates"] = ([known[7]] + list(g), 4, G[g][0])
    a, c = next((a, c) for a in sorted(g for g in G if len(g) == 2 and good(g)) if G[a][1] != 0.0 and G[a[1:]][1] != 0.0
                for c in known[20:] if (a[1], c) not in G)
    out["back_off_through_two_contexts"] = (list(a) + [c], 3,
                                            np.float32(np.float32(G[(c,)][0] + G[a[1:]][1]) + G[a][1]))
    x, y, c = next((x, y, c) for x in known[30:] for y in known[40:50] for c in known[50:60]
                   if (x, y) not in G and (y, c) not in G and G[(y,)][1] != 0.0)
    out["back_off_stops_at_a_missing_context"] = ([x, y, c], 3, np.float32(G[(c,)][0] + G[(y,)][1]))
    g = next(g for g in tri if g[1:] not in G and G[g[:2]][1] != 0.0)
    out["suffix_incomplete"] = (list(g), 3, np.float32(np.float32(G[g[2:]][0] + G[g[1:2]][1]) + G[g[:2]][1]))
    out["unk_word"] = ([known[11], next(w for w in words if w not in b.ids)], 3, None)
    both = next(w for w in known if any(v != w and v.startswith(w) for v in words))
    out["word_and_prefix"] = ([known[2], both, known[9], both], 4, None)
    # no listed 0.000000 on the way: at order 2 a path is read by decoder.lm.LM, which backs off from those
    g = next(g for g in tri if g[1:] in G and abs(float(G[g][0]) - float(G[g[1:]][0])) > 1.0
             and all(G.get(k, (1.0,))[0] != 0.0 for k in (("<s>", g[0]), g[:2], g[1:])))
    out["trigram_not_bigram"] = (list(g), 3, G[g][0])
    out["trigram_read_as_bigram"] = (list(g), 2, G[g[1:]][0])
    _CACHE["forced"] = out
    return out


FORCED = ["start", "listed_trigram", "listed_4gram", "history_truncates", "back_off_through_two_contexts",
          "back_off_stops_at_a_missing_context", "suffix_incomplete", "unk_word", "word_and_prefix",
          "trigram_not_bigram", "trigram_read_as_bigram"]


@pytest.mark.parametrize("what", FORCED)
def test_lm_terms_on_forced_paths(what):
    """one finite symbol per frame, the last frame space or blank, nbest 2: key(P+space) - key(P) is the
    space's log-probability minus the blank's plus alpha * P(w | h) + beta.  "trigram_not_bigram" and
    "trigram_read_as_bigram" are one sentence on one file: order 3 scores its last word with the listed
    trigram, order 2 with the bigram, more than 1 apart -- what a bigram-only decoder silently did to a
    trigram file."""
    import ctc_fast
    chars, words = chars_words()
    sent, order, expect = forced_cases()[what]
    sent = [w for w in sent if w != "<s>"]
    assert float(np.float32(ALPHA)) != ALPHA
    d, _, _ = device_lexicon(order)
    b = brute(order)
    rs = np.random.RandomState(len(what))
    syms = []
    for k, w in enumerate(sent):
        syms += ([SPACE] if k else []) + spell(chars, w)
    frames = []
    for s in syms:
        if frames and frames[-1] == s:
            frames.append(0)
        frames.append(s)
    T = len(frames) + 1
    lp = np.full((A, T), NEG)
    vals = -(0.05 + 2.0 * rs.rand(T + 1))
    lp[frames, np.arange(T - 1)] = vals[:T - 1]
    lp[SPACE, T - 1], lp[0, T - 1] = vals[T - 1], vals[T]
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=d, beam=8, alpha=ALPHA, beta=BETA, nbest=2)
    by_len = {len(h): (list(h), s) for h, s in zip(hyps[0], scores[0])}
    assert sorted(by_len) == [len(syms), len(syms) + 1], by_len
    (P, key_p), (Q, key_q) = by_len[len(syms)], by_len[len(syms) + 1]
    assert P == syms and Q == syms + [SPACE]
    names = [w if w in b.ids else "<UNK>" for w in sent]
    hist = ["<s>"]
    terms = []
    for w in names:
        terms.append(float(b.prob(hist, w)))
        hist.append(w)
    if expect is not None:
        assert terms[-1] == float(expect), (what, terms[-1], expect)
    if what == "unk_word":
        assert names[-1] == "<UNK>" and d.lm.get_word_id(sent[-1]) == d.lm.unk
    if what == "history_truncates":
        assert len(sent) == 5 and order == 4
    if what.startswith("trigram"):
        other = forced_cases()["trigram_read_as_bigram" if order == 3 else "trigram_not_bigram"][2]
        assert abs(terms[-1] - float(other)) > 1.0
    want = lp[SPACE, T - 1] - lp[0, T - 1] + ALPHA * terms[-1] + BETA
    print("%s (order %d, '%s'): key difference %.17g, closed form %.17g" % (what, order, " ".join(sent), key_q - key_p, want))
    assert abs((key_q - key_p) - want) <= 1e-12 * abs(key_q), (key_q - key_p, want)
    closed = float(np.sum(vals[:T])) + ALPHA * sum(terms) + BETA * len(sent)
    assert abs(key_q - closed) <= tol(closed), (key_q, closed)
    closed_p = float(np.sum(vals[:T - 1])) + vals[T] + ALPHA * sum(terms[:-1]) + BETA * (len(sent) - 1)
    assert abs(key_p - closed_p) <= tol(closed_p), (key_p, closed_p)


# ---- 4. the lexicon property in the corners of the ABI -------------------------------------------

def fixture_utts(rs, Ts, dt=np.float64):
    return [posteriors(rs, T).astype(dt) if T else np.zeros((A, 0), dtype=dt) for T in Ts]


def test_fewer_live_candidates_than_beam():
    import ctc_fast
    chars, _ = chars_words()
    A8, beam = 8, 64
    chars_a = {k: v for k, v in chars.items() if v < A8}
    d = ctc_fast.DecodeLexicon(["at", "ate", "no"], chars_a, ARPA4, "[space]", A=A8, order=3)
    child, word = d.tree.flatten(A8)
    b = brute(3)
    rs = np.random.RandomState(64)
    for T in (1, 2, 4):
        lp = logsoftmax(0.4 * rs.randn(A8, T))
        top = ngm.decode(lp, child, word, b.prob_ids, d.lm.start, SPACE, 3, beam=beam, alpha=ALPHA, beta=BETA,
                         nbest=beam)
        live = len(top)
        assert 1 < live < beam
        hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=d, beam=beam, alpha=ALPHA, beta=BETA,
                                                          nbest=beam)
        keys = [k for _, k in top]
        for n in range(live):
            assert abs(scores[0, n] - keys[n]) <= tol(keys[n]), (T, n)
            check_lexicon_property(hyps[0][n], child, word)
        for n in clear_ranks(keys):
            assert list(hyps[0][n]) == list(top[n][0]), (T, n)
        assert sorted(tuple(int(c) for c in h) for h in hyps[0][:live]) == sorted(p for p, _ in top)
        for n in range(live, beam):
            assert len(hyps[0][n]) == 0 and scores[0, n] == NEG, (T, n)


def test_t0_and_t1():
    import ctc_fast
    d, child, word = device_lexicon(4, "small")
    lp = fixture_utts(np.random.RandomState(2), (1,))[0]
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([np.zeros((A, 0)), lp], lexicon=d, beam=40, alpha=1.3,
                                                      beta=BETA, nbest=2)
    assert len(hyps[0][0]) == 0 and scores[0, 0] == 0.0 and scores[0, 1] == NEG and len(hyps[0][1]) == 0
    top = model_top(lp, 4, 40, 2, "small", alpha=1.3)
    for n in range(2):
        assert abs(scores[1, n] - top[n][1]) <= tol(top[n][1])
        check_lexicon_property(hyps[1][n], child, word)
    if top[0][1] - top[1][1] > tol(top[0][1]) + tol(top[1][1]):
        assert list(hyps[1][0]) == list(top[0][0])


def test_batch_composition_and_order():
    import ctc_fast
    d, child, word = device_lexicon(4)
    utts = fixture_utts(np.random.RandomState(11), (50, 1, 120, 0, 77, 200))
    kw = dict(lexicon=d, beam=24, alpha=ALPHA, beta=BETA)
    singles = [ctc_fast.decode_lexicon_beam_batch([u], **kw) for u in utts]
    hyps, scores = ctc_fast.decode_lexicon_beam_batch(utts, **kw)
    rh, rsc = ctc_fast.decode_lexicon_beam_batch(utts[::-1], **kw)
    for i, (sh, ss) in enumerate(singles):
        assert list(hyps[i]) == list(sh[0]) and scores[i] == ss[0]
        assert list(rh[len(utts) - 1 - i]) == list(sh[0]) and rsc[len(utts) - 1 - i] == ss[0]
        check_lexicon_property(hyps[i], child, word)
    top = model_top(utts[4], 4, 24, 1)
    assert abs(scores[4] - top[0][1]) <= tol(top[0][1])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ld_and_frame_offsets(dt):
    """ld > A with NaN in the padding columns, utterances in shuffled order with NaN-filled gaps"""
    import ctc_fast
    ld, beam, nbest = 48, 24, 3
    d, child, word = device_lexicon(3)
    utts = fixture_utts(np.random.RandomState(77), (60, 1, 33, 0, 90, 17), dt)
    T_b = [u.shape[1] for u in utts]
    order = [4, 0, 5, 2, 3, 1]
    gaps = [3, 0, 7, 1, 0, 5]
    host = np.full((sum(T_b) + sum(gaps) + 4, ld), np.nan, dtype=dt)
    frame_off = [0] * len(utts)
    row = 2
    for i, gap in zip(order, gaps):
        row += gap
        frame_off[i] = row
        host[row:row + T_b[i], :A] = utts[i].T
        row += T_b[i]
    assert sorted(frame_off) != frame_off
    hyps, scores, lens, _, _ = raw_decode("lexbeam", host, ld, A, T_b, frame_off, beam, nbest, d, ALPHA, BETA)
    ph, ps = ctc_fast.decode_lexicon_beam_batch(utts, lexicon=d, beam=beam, alpha=ALPHA, beta=BETA, nbest=nbest)
    np.testing.assert_array_equal(scores, ps)
    assert not np.isnan(scores).any()
    for i in range(len(utts)):
        for n in range(nbest):
            np.testing.assert_array_equal(hyps[i][n], ph[i][n])
            check_lexicon_property(hyps[i][n], child, word)
    assert max(len(h[0]) for h in hyps) > 5


@pytest.mark.parametrize("nbest", [1, 16])
def test_exact_workspace_and_guarded_outputs(nbest):
    """nothing outside the workspace of exactly the advertised size, ids, lengths and scores is
    written; the workspace is what the bigram lexicon of the same shape asks for"""
    import ctc_fast
    import ctypes
    import _sctc
    beam = 16
    d, child, word = device_lexicon(4, "small")
    utts = fixture_utts(np.random.RandomState(78), (0, 150, 1, 0, 37, 1, 220))
    T_b = [u.shape[1] for u in utts]
    host = np.ascontiguousarray(np.concatenate([u.T for u in utts], axis=0))
    frame_off = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    hyps, scores, lens, outside, nbytes = raw_decode("lexbeam", host, A, A, T_b, frame_off, beam, nbest, d, ALPHA, BETA,
                                                     guard=4096)
    assert outside.size >= 5 * 4096 and np.all(outside == PATTERN)
    fixed = 24 * beam * A + 255                                       # per utterance, each array 256-byte aligned
    assert nbytes <= 4096 + sum(3 * 256 + fixed + 4 * beam * T for T in T_b)
    ph, ps = ctc_fast.decode_lexicon_beam_batch(utts, lexicon=d, beam=beam, alpha=ALPHA, beta=BETA, nbest=nbest)
    np.testing.assert_array_equal(scores, np.asarray(ps).reshape(len(utts), nbest))
    for i in range(len(utts)):
        want = ph[i] if nbest > 1 else [ph[i]]
        for n in range(nbest):
            np.testing.assert_array_equal(hyps[i][n], want[n])
            check_lexicon_property(hyps[i][n], child, word)
    assert scores[0, 0] == 0.0 and lens[0, 0] == 0 and (nbest == 1 or scores[0, 1] == NEG)


def test_neg_inf_frame_kills_everything():
    import ctc_fast
    d, _, _ = device_lexicon(4, "small")
    lp = fixture_utts(np.random.RandomState(9), (40,))[0]
    lp[:, 17] = NEG
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=d, beam=16, alpha=ALPHA, beta=BETA, nbest=4)
    assert not np.isnan(scores).any() and np.all(scores == NEG)


def test_handles_count_their_tables_and_the_reference_surface():
    import ctc_fast
    from decoder import bg_decoder
    d4, child, word = device_lexicon(4)
    d3, _, _ = device_lexicon(3)
    keys = d4.lm.pack()[0]
    assert d4.device_bytes >= child.size * 4 + 20 * keys.shape[0]         # key, value, back-off and id per slot
    assert d3.device_bytes >= child.size * 4 + 20 * d3.lm.pack()[0].shape[0]
    # the reference-named surface with an NgramLM: the same search
    lp = posteriors(np.random.RandomState(5), 50)
    hyp, score = bg_decoder.decode_bg_lm(np.asfortranarray(lp), d4.tree, d4.lm, 16, ALPHA, BETA)
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=d4, beam=16, alpha=ALPHA, beta=BETA)
    assert hyp == [int(c) for c in hyps[0]] and score == scores[0]


# ---- 5. runDecode.py --method bg --word-lm-order 4 -----------------------------------------------

def test_run_decode_bg_order_4_end_to_end(tmp_path):
    import ctc_fast
    import dataLoader as dl
    import runDecode
    import writeLikelihoods as wl
    from decoder import decoder_utils
    from nnets import brnnet
    rs = np.random.RandomState(0)
    raw = img = 12
    A6 = 6                                           # blank, [space], a, e, [laughter], t
    data = tmp_path / "data"
    data.mkdir()
    refs = [[2, 5, 1, 3, 2, 5], [5, 3, 2], [4, 1, 2, 5, 3], [3, 2, 5, 1, 2], [2, 1, 2, 5]]
    utts = [("u%d" % i, int(rs.randint(14, 30)), r) for i, r in enumerate(refs)]
    write_shard(data, 1, utts, raw, rs)
    net = brnnet.NNet(img, A6, 32, 3, 40, train=False, temporalLayer=2)
    np.random.seed(1)
    net.initParams()
    loader = dl.DataLoader(str(data) + "/", raw, img)
    lik = tmp_path / "lik"
    lik.mkdir()
    wl.writeLogLikes(loader, net, 1, str(lik), writePickle=True)
    chars = tmp_path / "chars.txt"
    chars.write_text("".join(l for l in open(CHARS).readlines()[:A6 - 1]))
    words = tmp_path / "words.txt"
    lexicon = ["at", "ate", "tea", "eat", "a", "tat", "teat", "t", "ta", "e"]
    words.write_text("\n".join(lexicon) + "\n")
    out = tmp_path / "hyps.txt"
    args = ["--method", "bg", "--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", str(chars),
            "--alis", str(data / "alis1.txt"), "--words", str(words), "--word-lm", ARPA4, "--word-lm-order", "4",
            "--specials", "[laughter]", "--out", str(out), "--beam", "8", "--alpha", "0.8", "--beta", "0.37",
            "--batch", "2"]
    cer, wer = runDecode.main(args)
    lines = out.read_text().splitlines()
    assert len(lines) == 5 and np.isfinite(cer) and np.isfinite(wer) and cer >= 0 and wer >= 0
    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    cmap = decoder_utils.load_chars(str(chars))
    d4 = ctc_fast.DecodeLexicon(lexicon, cmap, ARPA4, "[space]", specials=["[laughter]"], order=4)
    d2 = ctc_fast.DecodeLexicon(lexicon, cmap, ARPA4, "[space]", specials=["[laughter]"])
    alis = runDecode.load_alis(str(data / "alis1.txt"), str(chars))
    ce = cn = we = wn = 0
    allowed = set(lexicon) | {"[laughter]"}
    for l in lines:
        parts = l.split(" ", 2)
        hyps, scores = ctc_fast.decode_lexicon_beam_batch([pk[parts[0]]], lexicon=d4, beam=8, alpha=0.8, beta=0.37)
        toks = decoder_utils.int_to_char(hyps[0], cmap)
        text = decoder_utils.collapse_seq(toks)
        assert float(parts[1]) == pytest.approx(scores[0], abs=1e-6)
        assert (parts[2] if len(parts) > 2 else "") == text
        assert all(w in allowed for w in text.split()[:-1])
        ref = alis[parts[0]]
        ce += runDecode.edit_distance(ref, toks)
        cn += len(ref)
        ref_words = decoder_utils.collapse_seq(ref).split()
        we += runDecode.edit_distance(ref_words, text.split())
        wn += len(ref_words)
    assert cer == ce / float(cn) and wer == we / float(wn)
    # the default order is 2: without the option the file is read as the bigram it was always read as
    out2 = tmp_path / "hyps2.txt"
    runDecode.main([a for a in args if a not in ("--word-lm-order", "4")] + ["--out", str(out2)])
    for l in out2.read_text().splitlines():
        parts = l.split(" ", 2)
        hyps, scores = ctc_fast.decode_lexicon_beam_batch([pk[parts[0]]], lexicon=d2, beam=8, alpha=0.8, beta=0.37)
        assert float(parts[1]) == pytest.approx(scores[0], abs=1e-6)
