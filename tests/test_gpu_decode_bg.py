"""GPU checks of the lexicon-constrained word-bigram beam search (csrc/ctc_beam.hip
``ctc_lexbeam_kernel``) through the public Python and C surfaces: the reference's
own results (tests/golden/decode_bg_ref.npz), the Python restatement (tests/lex_beam_model.py) at
size, the lexicon property of every returned hypothesis, bigram terms read off forced paths, a beam
with fewer live candidates than its width, the ABI corners the character decoder is held to, and
runDecode.py --method bg."""
import os
import pickle

import numpy as np
import pytest

from tests import lex_beam_model
from tests.beam_harness import PATTERN, raw_decode
from tests.beam_trace import logsoftmax, tol
from tests.test_dataloader import write_shard
from tests.test_decode_bg_cpu import ARPA, CHARS, GOLDEN, WORDS, fixture_lexicon

pytestmark = pytest.mark.gpu

NEG = float("-inf")
SPACE = 1


def objects():
    from decoder import decoder_utils, lm as lm_mod
    return decoder_utils.load_chars(CHARS), decoder_utils.load_words(WORDS), lm_mod.LM(ARPA)


_LEX = {}


def fixture_device_lexicon(A, size):
    """(DecodeLexicon, restatement arguments, words, specials) of a fixture lexicon"""
    import ctc_fast
    if (A, size) not in _LEX:
        chars, words, lm = objects()
        lex, sp = fixture_lexicon(words, A, size)
        chars_a = {k: v for k, v in chars.items() if v < A}
        d = ctc_fast.DecodeLexicon(lex, chars_a, lm, "[space]", specials=sp, A=A)
        _LEX[(A, size)] = (d, lex_beam_model.from_objects(d.tree, lm, A), lex, sp)
    return _LEX[(A, size)]


def word_path(rs, chars, lexicon, T, blank_p=0.25):
    """frame labels of a random word sequence (runs of 1..3 frames, blanks between equal neighbours)"""
    path = []
    while len(path) < T:
        syms = [chars[ch] for ch in lexicon[rs.randint(len(lexicon))]] + [SPACE]
        for s in syms:
            if (path and path[-1] == s) or rs.rand() < blank_p:
                path += [0] * rs.randint(1, 3)
            path += [s] * rs.randint(1, 4)
    return np.array(path[:T])


def peaked_words(rs, A, T, chars, lexicon, sharp=6.0):
    x = 1.5 * rs.randn(A, T)
    x[word_path(rs, chars, lexicon, T), np.arange(T)] += sharp
    return logsoftmax(x)


def check_lexicon_property(hyp, child, word):
    """split at the space: every complete segment is a word (or special), the trailing segment is
    empty or a prefix in the tree, no leading space, no double space"""
    node = 0
    for i, c in enumerate(hyp):
        c = int(c)
        if c == SPACE:
            assert i > 0 and hyp[i - 1] != SPACE, "leading or double space"
            assert word[node] >= 0, "a space after a non-word"
            node = 0
        else:
            node = child[node, c]
            assert node > 0, "a spelling outside the tree"


# ---- 1. the reference ----------------------------------------------------------------------------

def test_against_reference_golden():
    import ctc_fast
    from decoder import bg_decoder
    _, _, lm = objects()
    z = np.load(os.path.join(GOLDEN, "decode_bg_ref.npz"))
    n = int(z["n"])
    assert n >= 40
    skipped = 0
    for i in range(n):
        A, T, beam, alpha, beta = z["cfg%d" % i]
        A, T, beam = int(A), int(T), int(beam)
        dlex, model, _, _ = fixture_device_lexicon(A, str(z["lex%d" % i]))
        lp = z["lp%d" % i]
        ref, margin = float(z["score%d" % i]), float(z["margin%d" % i])
        hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, beam=beam, alpha=alpha, beta=beta)
        print("case %d: score %.9f reference %.9f margin %.3g" % (i, scores[0], ref, margin))
        assert abs(scores[0] - ref) <= tol(ref), (i, scores[0], ref)
        if margin >= 1e-6:
            assert list(hyps[0]) == list(z["hyp%d" % i]), i
        else:
            skipped += 1
        check_lexicon_property(hyps[0], model[0], model[1])
        # the reference-named surface: the same tree and LM objects, float64 Fortran input
        if i % 6 == 0:
            hyp, score = bg_decoder.decode_bg_lm(np.asfortranarray(lp), dlex.tree, lm, beam, alpha, beta)
            assert hyp == [int(c) for c in hyps[0]] and score == scores[0]
    assert skipped <= 0.05 * n


# ---- 2. the restatement at size, 3. the lexicon property -----------------------------------------

@pytest.fixture(scope="module")
def big_lexicon(tmp_path_factory):
    """about 20 000 synthetic words over the letters of chars.txt (A = 33) and a word bigram"""
    import ctc_fast
    from decoder import decoder_utils, lm as lm_mod
    rs = np.random.RandomState(20000)
    chars = {k: v for k, v in decoder_utils.load_chars(CHARS).items() if v < 33}
    letters = [k for k, v in chars.items() if len(k) == 1]
    words = sorted(set("".join(rs.choice(letters, size=rs.randint(2, 10))) for _ in range(22600)))
    rs.shuffle(words)
    vocab = ["<s>", "</s>", "<UNK>", "[noise]"] + words[:-200]          # 200 words are unknown to the LM
    d = tmp_path_factory.mktemp("biglex")
    lines = ["\\data\\", "ngram 1=%d" % len(vocab), "ngram 2=60000", "", "\\1-grams:"]
    for w in vocab:
        lines.append("%.6f\t%s\t%.6f" % (-99.0 if w == "<s>" else -(1 + 4 * rs.rand()), w, -(0.1 + rs.rand())))
    lines += ["", "\\2-grams:"]
    pairs = set()
    while len(pairs) < 60000:
        a = 0 if rs.rand() < 0.05 else rs.randint(2, len(vocab))
        pairs.add((a, rs.randint(1, len(vocab))))
    for a, b in sorted(pairs):
        lines.append("%.6f\t%s %s" % (-(0.1 + 3 * rs.rand()), vocab[a], vocab[b]))
    lines += ["", "\\end\\", ""]
    arpa = d / "big.arpa"
    arpa.write_text("\n".join(lines))
    lm = lm_mod.LM(str(arpa))
    specials = ["[laughter]", "[noise]"]
    dlex = ctc_fast.DecodeLexicon(words, chars, lm, "[space]", specials=specials, A=33)
    return dlex, lex_beam_model.from_objects(dlex.tree, lm, 33), chars, words


@pytest.mark.parametrize("T,beam", [(1000, 40), (1000, 150), (1000, 256), (2000, 40), (2000, 150), (2000, 256)])
def test_against_restatement_at_size(big_lexicon, T, beam):
    import ctc_fast
    dlex, model, chars, words = big_lexicon
    assert len(words) >= 19000 and dlex.nodes > 50000
    rs = np.random.RandomState(T + beam)
    lp = peaked_words(rs, 33, T, chars, words, sharp=5.0)
    top = lex_beam_model.decode(lp, *model, beam=beam, alpha=0.8, beta=0.37, nbest=beam)
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, beam=beam, alpha=0.8, beta=0.37,
                                                      nbest=beam)
    assert len(top) == beam
    keys = [k for _, k in top]
    worst = max(abs(scores[0, n] - keys[n]) / tol(keys[n]) for n in range(beam))
    print("T %d beam %d: worst key difference %.3g of the tolerance" % (T, beam, worst))
    compared = 0
    for n in range(beam):
        assert abs(scores[0, n] - keys[n]) <= tol(keys[n]), (n, scores[0, n], keys[n])
        check_lexicon_property(hyps[0][n], model[0], model[1])
        clear = all(abs(keys[n] - keys[m]) > tol(keys[n]) + tol(keys[m]) for m in (n - 1, n + 1) if 0 <= m < beam)
        if clear:
            assert list(hyps[0][n]) == list(top[n][0]), n
            compared += 1
    print("hypotheses compared: %d of %d" % (compared, beam))
    assert compared > 0 and len(hyps[0][0]) > T // 10


def test_lexicon_of_200000_nodes():
    """the dense child table at the size DESIGN.md §4.6 promises: more than 200 000 nodes, A = 35"""
    import ctc_fast
    from decoder import decoder_utils
    chars, _, lm = objects()
    A = 35
    rs = np.random.RandomState(200000)
    letters = [k for k in chars if len(k) == 1 and k != "&"]
    words = sorted(set("".join(rs.choice(letters, size=rs.randint(3, 12))) for _ in range(50000)))
    dlex = ctc_fast.DecodeLexicon(words, chars, lm, "[space]", specials=["[noise]"], A=A)
    assert dlex.nodes > 200000 and dlex.device_bytes >= dlex.nodes * A * 4
    model = lex_beam_model.from_objects(dlex.tree, lm, A)
    lp = peaked_words(rs, A, 150, chars, words, sharp=5.0)
    top = lex_beam_model.decode(lp, *model, beam=40, alpha=0.8, beta=0.37, nbest=2)
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, beam=40, alpha=0.8, beta=0.37, nbest=2)
    for n in range(2):
        assert abs(scores[0, n] - top[n][1]) <= tol(top[n][1])
    if top[0][1] - top[1][1] > tol(top[0][1]) + tol(top[1][1]):
        assert list(hyps[0][0]) == list(top[0][0])
    check_lexicon_property(hyps[0][0], model[0], model[1])
    assert len(hyps[0][0]) > 15


# ---- 4. bigram terms read off forced paths -------------------------------------------------------

def forced_sentences():
    """{what: [words]}: the last word's bigram (previous word, word) is the term under test"""
    chars, words, lm = objects()
    known = [w for w in words if w in lm.word_to_int]
    ids = lm.word_to_int
    out = {"start": [known[3]]}
    out["listed"] = next([a, b] for a in known for b in known if lm.bg.get((ids[a], ids[b]), 0.0) != 0.0)
    out["backed_off"] = next([a, b] for a in known[5:] for b in known[7:] if (ids[a], ids[b]) not in lm.bg)
    out["zero_quirk"] = next([a, b] for a in known for b in known
                             if (ids[a], ids[b]) in lm.bg and lm.bg[(ids[a], ids[b])] == 0.0)
    unk = next(w for w in words if w not in ids)
    out["unk_word"] = [known[11], unk]
    both = next(w for w in known if any(v != w and v.startswith(w) for v in words))
    out["word_and_prefix"] = [known[2], both, known[9], both]
    return out


@pytest.mark.parametrize("what", ["start", "listed", "backed_off", "zero_quirk", "unk_word", "word_and_prefix"])
def test_bigram_terms_on_forced_paths(what):
    import ctc_fast
    chars, words, lm = objects()
    A, alpha, beta = 35, 0.8, 0.37
    assert float(np.float32(alpha)) != alpha
    dlex, _, _, _ = fixture_device_lexicon(A, "large")
    sent = forced_sentences()[what]
    rs = np.random.RandomState(len(what))
    syms = []
    for k, w in enumerate(sent):
        if k:
            syms.append(SPACE)
        syms += [chars[ch] for ch in w]
    frames = []
    for s in syms:
        if frames and frames[-1] == s:
            frames.append(0)
        frames.append(s)
    T = len(frames) + 1
    lp = np.full((A, T), NEG)
    vals = -(0.05 + 2.0 * rs.rand(T + 1))
    lp[frames, np.arange(T - 1)] = vals[:T - 1]
    lp[SPACE, T - 1], lp[0, T - 1] = vals[T - 1], vals[T]            # the last frame: space or blank
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, beam=8, alpha=alpha, beta=beta, nbest=2)
    by_len = {len(h): (list(h), s) for h, s in zip(hyps[0], scores[0])}
    assert sorted(by_len) == [len(syms), len(syms) + 1], by_len
    (P, key_p), (Q, key_q) = by_len[len(syms)], by_len[len(syms) + 1]
    assert P == syms and Q == syms + [SPACE]
    wid = [lm.get_word_id(w) for w in sent]
    prev = lm.start if len(sent) == 1 else wid[-2]
    bg = float(lm.bg_prob(prev, wid[-1]))
    if what == "zero_quirk":
        assert lm.bg[(prev, wid[-1])] == 0.0 and bg == float(np.float32(lm.bo[prev] + lm.ug[wid[-1]])) != 0.0
    if what == "unk_word":
        assert wid[-1] == lm.unk
    want = lp[SPACE, T - 1] - lp[0, T - 1] + alpha * bg + beta
    print("%s: key difference %.17g, closed form %.17g" % (what, key_q - key_p, want))
    assert abs((key_q - key_p) - want) <= 1e-12 * abs(key_q), (key_q - key_p, want)
    # the whole score: sum of the path's log-probabilities, alpha * every bigram, beta per word
    bgs = [float(lm.bg_prob(a, b)) for a, b in zip([lm.start] + wid[:-1], wid)]
    closed = float(np.sum(vals[:T])) + alpha * sum(bgs) + beta * len(sent)
    assert abs(key_q - closed) <= tol(closed), (key_q, closed)
    closed_p = float(np.sum(vals[:T - 1])) + vals[T] + alpha * sum(bgs[:-1]) + beta * (len(sent) - 1)
    assert abs(key_p - closed_p) <= tol(closed_p), (key_p, closed_p)


# ---- 5. fewer live candidates than the beam is wide ----------------------------------------------

def test_fewer_live_candidates_than_beam():
    import ctc_fast
    chars, _, lm = objects()
    A, beam = 8, 64
    chars_a = {k: v for k, v in chars.items() if v < A}
    dlex = ctc_fast.DecodeLexicon(["at", "ate", "no"], chars_a, lm, "[space]", A=A)
    model = lex_beam_model.from_objects(dlex.tree, lm, A)
    rs = np.random.RandomState(64)
    for T in (1, 2, 4):
        lp = logsoftmax(0.4 * rs.randn(A, T))
        top = lex_beam_model.decode(lp, *model, beam=beam, alpha=0.8, beta=0.37, nbest=beam)
        live = len(top)
        assert 1 < live < beam
        hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, beam=beam, alpha=0.8, beta=0.37,
                                                          nbest=beam)
        for n in range(live):
            assert abs(scores[0, n] - top[n][1]) <= tol(top[n][1]), (T, n)
            check_lexicon_property(hyps[0][n], model[0], model[1])
        keys = [k for _, k in top]
        for n in range(live):
            if all(abs(keys[n] - keys[m]) > tol(keys[n]) + tol(keys[m]) for m in (n - 1, n + 1) if 0 <= m < live):
                assert list(hyps[0][n]) == list(top[n][0]), (T, n)
        assert sorted(tuple(int(c) for c in h) for h in hyps[0][:live]) == sorted(p for p, _ in top)
        for n in range(live, beam):
            assert len(hyps[0][n]) == 0 and scores[0, n] == NEG, (T, n)


# ---- 6. the ABI corners --------------------------------------------------------------------------

def fixture_utts(rs, A, Ts, dt=np.float64):
    chars, _, _ = objects()
    _, _, lex, _ = fixture_device_lexicon(A, "large")
    return [peaked_words(rs, A, T, chars, lex).astype(dt) if T else np.zeros((A, 0), dtype=dt) for T in Ts]


def test_float32_and_float64_device_input():
    import torch
    import ctc_fast
    A = 35
    dlex, _, _, _ = fixture_device_lexicon(A, "large")
    utts = fixture_utts(np.random.RandomState(5), A, (90, 40, 130), np.float32)
    lengths = [u.shape[1] for u in utts]
    rows = np.concatenate([u.T for u in utts], axis=0)
    kw = dict(lexicon=dlex, beam=32, alpha=0.8, beta=0.37)
    h32, s32 = ctc_fast.decode_lexicon_beam_batch(torch.from_numpy(rows).cuda(), lengths, **kw)
    h64, s64 = ctc_fast.decode_lexicon_beam_batch(torch.from_numpy(rows.astype(np.float64)).cuda(), lengths, **kw)
    hl, sl = ctc_fast.decode_lexicon_beam_batch(utts, **kw)
    for b in range(3):
        assert list(h32[b]) == list(h64[b]) == list(hl[b]) and len(h32[b]) > 5
    np.testing.assert_array_equal(s32, s64)
    np.testing.assert_array_equal(s32, sl)


def test_t0_and_t1():
    import ctc_fast
    A = 35
    dlex, model, _, _ = fixture_device_lexicon(A, "small")
    lp = fixture_utts(np.random.RandomState(2), A, (1,))[0]
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([np.zeros((A, 0)), lp], lexicon=dlex, beam=40, alpha=1.3,
                                                      beta=0.37, nbest=2)
    assert len(hyps[0][0]) == 0 and scores[0, 0] == 0.0 and scores[0, 1] == NEG and len(hyps[0][1]) == 0
    top = lex_beam_model.decode(lp, *model, beam=40, alpha=1.3, beta=0.37, nbest=2)
    for n in range(2):
        assert abs(scores[1, n] - top[n][1]) <= tol(top[n][1])
    if top[0][1] - top[1][1] >= 1e-6:
        assert list(hyps[1][0]) == list(top[0][0])


def test_batch_composition_and_order():
    import ctc_fast
    A = 33
    dlex, _, _, _ = fixture_device_lexicon(A, "large")
    utts = fixture_utts(np.random.RandomState(11), A, (50, 1, 120, 0, 77, 200))
    kw = dict(lexicon=dlex, beam=24, alpha=0.8, beta=0.37)
    singles = [ctc_fast.decode_lexicon_beam_batch([u], **kw) for u in utts]
    hyps, scores = ctc_fast.decode_lexicon_beam_batch(utts, **kw)
    rh, rsc = ctc_fast.decode_lexicon_beam_batch(utts[::-1], **kw)
    for b, (sh, ss) in enumerate(singles):
        assert list(hyps[b]) == list(sh[0]) and scores[b] == ss[0]
        assert list(rh[len(utts) - 1 - b]) == list(sh[0]) and rsc[len(utts) - 1 - b] == ss[0]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ld_and_frame_offsets(dt):
    """ld > A with NaN in the padding columns, utterances in shuffled order with NaN-filled gaps"""
    import ctc_fast
    A, ld, beam, nbest = 35, 48, 24, 3
    dlex, _, _, _ = fixture_device_lexicon(A, "large")
    utts = fixture_utts(np.random.RandomState(77), A, (60, 1, 33, 0, 90, 17), dt)
    T_b = [u.shape[1] for u in utts]
    order = [4, 0, 5, 2, 3, 1]
    gaps = [3, 0, 7, 1, 0, 5]
    host = np.full((sum(T_b) + sum(gaps) + 4, ld), np.nan, dtype=dt)
    frame_off = [0] * len(utts)
    row = 2
    for b, gap in zip(order, gaps):
        row += gap
        frame_off[b] = row
        host[row:row + T_b[b], :A] = utts[b].T
        row += T_b[b]
    assert sorted(frame_off) != frame_off
    hyps, scores, lens, _, _ = raw_decode("lexbeam", host, ld, A, T_b, frame_off, beam, nbest, dlex, 0.8, 0.37)
    ph, ps = ctc_fast.decode_lexicon_beam_batch(utts, lexicon=dlex, beam=beam, alpha=0.8, beta=0.37, nbest=nbest)
    np.testing.assert_array_equal(scores, ps)
    assert not np.isnan(scores).any()
    for b in range(len(utts)):
        for n in range(nbest):
            np.testing.assert_array_equal(hyps[b][n], ph[b][n])
    assert max(len(h[0]) for h in hyps) > 5


@pytest.mark.parametrize("nbest", [1, 16])
def test_exact_workspace_and_guarded_outputs(nbest):
    """nothing outside the workspace of exactly the advertised size, ids, lengths and scores is
    written: T = 0, T = 1 and long utterances mixed"""
    import ctc_fast
    A, beam = 35, 16
    dlex, _, _, _ = fixture_device_lexicon(A, "small")
    utts = fixture_utts(np.random.RandomState(78), A, (0, 150, 1, 0, 37, 1, 220))
    T_b = [u.shape[1] for u in utts]
    host = np.ascontiguousarray(np.concatenate([u.T for u in utts], axis=0))
    frame_off = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    hyps, scores, lens, outside, _ = raw_decode("lexbeam", host, A, A, T_b, frame_off, beam, nbest, dlex, 0.8, 0.37,
                                                guard=4096)
    assert outside.size >= 5 * 4096 and np.all(outside == PATTERN)
    ph, ps = ctc_fast.decode_lexicon_beam_batch(utts, lexicon=dlex, beam=beam, alpha=0.8, beta=0.37, nbest=nbest)
    np.testing.assert_array_equal(scores, np.asarray(ps).reshape(len(utts), nbest))
    for b in range(len(utts)):
        want = ph[b] if nbest > 1 else [ph[b]]
        for n in range(nbest):
            np.testing.assert_array_equal(hyps[b][n], want[n])
    assert scores[0, 0] == 0.0 and lens[0, 0] == 0 and (nbest == 1 or scores[0, 1] == NEG)


def test_limits_rejected():
    import ctc_fast
    A = 35
    dlex, _, _, _ = fixture_device_lexicon(A, "small")
    lp = fixture_utts(np.random.RandomState(0), A, (10,))[0]
    for kw in (dict(beam=257), dict(beam=0), dict(nbest=5, beam=4)):
        with pytest.raises(ValueError):
            ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, **kw)
    with pytest.raises(ValueError):
        ctc_fast.decode_lexicon_beam_batch([lp[:33]], lexicon=dlex)          # another alphabet than the lexicon's


def test_neg_inf_frame_kills_everything():
    import ctc_fast
    A = 35
    dlex, _, _, _ = fixture_device_lexicon(A, "small")
    lp = fixture_utts(np.random.RandomState(9), A, (40,))[0]
    lp[:, 17] = NEG
    hyps, scores = ctc_fast.decode_lexicon_beam_batch([lp], lexicon=dlex, beam=16, alpha=0.8, beta=0.37, nbest=4)
    assert not np.isnan(scores).any() and np.all(scores == NEG)


# ---- 7. runDecode.py --method bg -----------------------------------------------------------------

def test_run_decode_bg_end_to_end(tmp_path):
    import ctc_fast
    import dataLoader as dl
    import runDecode
    import writeLikelihoods as wl
    from decoder import decoder_utils
    from nnets import brnnet
    rs = np.random.RandomState(0)
    raw = img = 12
    A = 6                                            # blank, [space], a, e, [laughter], t
    data = tmp_path / "data"
    data.mkdir()
    refs = [[2, 5, 1, 3, 2, 5], [5, 3, 2], [4, 1, 2, 5, 3], [3, 2, 5, 1, 2], [2, 1, 2, 5]]
    utts = [("u%d" % i, int(rs.randint(14, 30)), r) for i, r in enumerate(refs)]
    write_shard(data, 1, utts, raw, rs)
    net = brnnet.NNet(img, A, 32, 3, 40, train=False, temporalLayer=2)
    np.random.seed(1)
    net.initParams()
    loader = dl.DataLoader(str(data) + "/", raw, img)
    lik = tmp_path / "lik"
    lik.mkdir()
    wl.writeLogLikes(loader, net, 1, str(lik), writePickle=True)
    chars = tmp_path / "chars.txt"
    chars.write_text("".join(l for l in open(CHARS).readlines()[:A - 1]))
    words = tmp_path / "words.txt"
    lexicon = ["at", "ate", "tea", "eat", "a", "tat", "teat"]
    words.write_text("\n".join(lexicon) + "\n")
    out = tmp_path / "hyps.txt"
    args = ["--method", "bg", "--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", str(chars),
            "--alis", str(data / "alis1.txt"), "--words", str(words), "--word-lm", ARPA, "--specials", "[laughter]",
            "--out", str(out), "--beam", "8", "--alpha", "0.8", "--beta", "0.37", "--batch", "2"]
    cer, wer = runDecode.main(args)
    lines = out.read_text().splitlines()
    assert len(lines) == 5 and np.isfinite(cer) and np.isfinite(wer) and cer >= 0 and wer >= 0
    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    cmap = decoder_utils.load_chars(str(chars))
    dlex = ctc_fast.DecodeLexicon(lexicon, cmap, ARPA, "[space]", specials=["[laughter]"])
    alis = runDecode.load_alis(str(data / "alis1.txt"), str(chars))
    ce = cn = we = wn = 0
    allowed = set(lexicon) | {"[laughter]"}
    for l in lines:
        parts = l.split(" ", 2)
        hyps, scores = ctc_fast.decode_lexicon_beam_batch([pk[parts[0]]], lexicon=dlex, beam=8, alpha=0.8, beta=0.37)
        toks = decoder_utils.int_to_char(hyps[0], cmap)
        text = decoder_utils.collapse_seq(toks)
        assert float(parts[1]) == pytest.approx(scores[0], abs=1e-6)
        assert (parts[2] if len(parts) > 2 else "") == text
        assert all(w in allowed for w in text.split()[:-1])           # words; the last one may be unfinished
        ref = alis[parts[0]]
        ce += runDecode.edit_distance(ref, toks)
        cn += len(ref)
        ref_words = decoder_utils.collapse_seq(ref).split()
        we += runDecode.edit_distance(ref_words, text.split())
        wn += len(ref_words)
    assert cer == ce / float(cn) and wer == we / float(wn)
    # the default method is untouched by the new options
    with pytest.raises(SystemExit):
        runDecode.main(["--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", str(chars),
                        "--alis", str(data / "alis1.txt"), "--out", str(out)])
