"""GPU checks of sctc_lm_score_batch (csrc/lm_score.hip, csrc/lm_score_plan.h) through
ctc_fast.lm_score_batch and ctc_fast.lm_perplexity.

The yardstick is the existing host route, untouched: a term is the entry of the row that ``lm.rows`` returns for the
prefix (the n-gram LM: ``ArpaLM.score_ids``), a sum is what ``ctc_fast.lm_sentence_scores`` returns.  Every
comparison is for equal bits (assert_array_equal): the device walks the sequences through the routines the rows come
from.  The yardstick of a model is computed once, for its longest list; a list of n sequences is the first n of it."""
import ctypes
import os

import numpy as np
import pytest

from tests.beam_harness import PATTERN, int_char_map
from tests import beam_trace as bt
from tests import test_gpu_decode_nn as NN
from tests import test_gpu_decode_rnn as RNN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEG = float("-inf")
A = 35
COUNTS = (1, 31, 32, 33, 65)
_NGRAM, _YARD = {}, {}

# (kind, model): the lengths every list starts with -- 0, 1, 2, K - 1, K, K + 1 around the window LM's K (the
# recurrent LM has no K: the fixture window's), order + 2 of the n-gram LMs -- and how many sequences the longest
# list has.  h1024: six sequences of at most 12 labels.
CASES = {
    ("rnn", "fix"): ([9, 0, 1, 2, 7, 8, 4, 7], 65),
    ("rnn", "h40"): ([9, 0, 1, 2, 7, 8, 4, 7], 65),
    ("rnn", "h1024"): ([12, 0, 1, 2, 5, 9], 6),
    ("nn", "fix"): ([9, 0, 1, 2, 7, 8, 4, 7], 65),
    ("nn", "k19"): ([20, 0, 1, 2, 18, 19, 4, 7], 65),
    ("ngram", "2g"): ([9, 0, 1, 2, 7, 8, 4, 7], 65),
    ("ngram", "5g"): ([9, 0, 1, 2, 3, 4, 5, 7], 65),
}


def dev_lm(kind, name):
    import ctc_fast
    if kind == "rnn":
        return RNN.dev_lm(name, A)
    if kind == "nn":
        return NN.dev_lm(name, A)
    if name not in _NGRAM:
        _NGRAM[name] = ctc_fast.DecodeLM(os.path.join(GOLDEN, "lm_char_%s.arpa" % name), int_char_map(), A)
    return _NGRAM[name]


def sequences(kind, name):
    head, n = CASES[kind, name]
    rs = np.random.RandomState(len(name) + 17 * len(kind))
    lens = head[:n] + [int(u) for u in rs.randint(0, 41, size=max(0, n - len(head)))]
    return [rs.randint(1, A, size=u).astype(np.int32) for u in lens]


def host_terms(lm, seqs):
    """the float32 term of every position by the host route: the entry of the prefix's row"""
    import ctc_fast
    if isinstance(lm, ctc_fast.DecodeLM):
        out = []
        for s in seqs:
            ctx, t = [lm.arpa.bos], []
            for c in s:
                w = int(lm.sym_words[int(c)])
                t.append(np.float32(lm.arpa.score_ids(ctx, w)))
                ctx.append(w)
            out.append(np.asarray(t, dtype=np.float32))
        return out
    prefixes = [tuple(int(c) for c in s[:i]) for s in seqs for i in range(len(s))]
    rows = lm.rows(prefixes) if prefixes else np.zeros((0, A), dtype=np.float32)
    out, k = [], 0
    for s in seqs:
        out.append(np.asarray([rows[k + i, int(c)] for i, c in enumerate(s)], dtype=np.float32))
        k += len(s)
    return out


def yardstick(kind, name):
    """(sequences, host terms, lm_sentence_scores) of a model's longest list, once"""
    import ctc_fast
    if (kind, name) not in _YARD:
        lm = dev_lm(kind, name)
        seqs = sequences(kind, name)
        _YARD[kind, name] = (seqs, host_terms(lm, seqs), ctc_fast.lm_sentence_scores(seqs, lm))
    return _YARD[kind, name]


# ---- 1. terms and sums against the host route, bit for bit --------------------------------------------------------

@pytest.mark.parametrize("kind,name", sorted(CASES))
def test_terms_equal_the_rows_and_sums_the_host_sums(kind, name):
    import ctc_fast
    lm = dev_lm(kind, name)
    seqs, terms, sums = yardstick(kind, name)
    assert {0, 1, 2} <= {len(s) for s in seqs}
    for n in COUNTS:
        if n > len(seqs) and n != COUNTS[0]:
            continue
        n = min(n, len(seqs))
        got_sums, got_terms = ctc_fast.lm_score_batch(seqs[:n], lm, terms=True)
        assert got_sums.dtype == np.float64 and got_sums.shape == (n,)
        for i in range(n):
            assert got_terms[i].dtype == np.float32
            np.testing.assert_array_equal(got_terms[i], terms[i], err_msg="%s %s: %d sequences, sequence %d" % (kind, name, n, i))
        np.testing.assert_array_equal(got_sums, sums[:n])
        # without a terms array the terms go through the workspace: the same sums
        np.testing.assert_array_equal(ctc_fast.lm_score_batch(seqs[:n], lm), sums[:n])
    whole = ctc_fast.lm_score_batch(seqs, lm)
    np.testing.assert_array_equal(whole, sums)
    assert whole[[i for i, s in enumerate(seqs) if len(s) == 0]].tolist() == [0.0] * sum(1 for s in seqs if len(s) == 0)


# ---- 2. composition: alone, in a batch, reversed, with a repeated offset; more tiles than resident blocks ---------

@pytest.mark.parametrize("kind,name", [("rnn", "fix"), ("nn", "fix"), ("ngram", "2g")])
def test_composition_beyond_the_resident_tiles(kind, name):
    import torch
    import _sctc
    import ctc_fast
    lm = dev_lm(kind, name)
    rs = np.random.RandomState(5)
    N = _sctc.LM_SCORE_TILE * _sctc.LM_SCORE_RESIDENT + 150       # 517 tiles of sequences, 1000-odd of positions
    seqs = [rs.randint(1, A, size=1 + (i * 7) % 3).astype(np.int32) for i in range(N)]
    assert sum(len(s) for s in seqs) > _sctc.LM_SCORE_TILE * _sctc.LM_SCORE_RESIDENT
    sums, terms = ctc_fast.lm_score_batch(seqs, lm, terms=True)
    rsums, rterms = ctc_fast.lm_score_batch(seqs[::-1], lm, terms=True)
    np.testing.assert_array_equal(rsums[::-1], sums)
    # alone: the first and last sequences, and the ones of one label that the recurrent path sorts into its last tiles
    ones = [i for i, s in enumerate(seqs) if len(s) == 1]
    picks = [0, 1, N - 1, ones[0], ones[-1], ones[len(ones) // 2]]
    asums, aterms = ctc_fast.lm_score_batch([seqs[i] for i in picks], lm, terms=True)
    for j, i in enumerate(picks):
        one_sum, one_terms = ctc_fast.lm_score_batch([seqs[i]], lm, terms=True)
        for other in (aterms[j], terms[i], rterms[N - 1 - i]):
            np.testing.assert_array_equal(one_terms[0], other)
        assert one_sum[0] == asums[j] == sums[i]
    # the device triple, read in place, with the offsets of the picks repeated
    U = np.asarray([len(s) for s in seqs], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(U)[:-1]])
    ids = torch.from_numpy(np.concatenate(seqs)).cuda()
    rep = np.asarray(picks + list(range(N)) + picks[::-1])
    tsums, tterms = ctc_fast.lm_score_batch((ids, U[rep], off[rep]), lm, terms=True, device=True)
    assert tsums.is_cuda and tterms.is_cuda and tterms.shape[0] == int(U[rep].sum())
    np.testing.assert_array_equal(tsums.cpu().numpy(), sums[rep])
    np.testing.assert_array_equal(tterms.cpu().numpy(), np.concatenate([terms[i] for i in rep]))


# ---- 3. in place on a search's device output ------------------------------------------------------------------------

def test_in_place_on_a_search_output():
    import ctc_fast
    lm = dev_lm("ngram", "2g")
    rnn = dev_lm("rnn", "fix")
    rs = np.random.RandomState(11)
    T_b = [30, 17, 24]
    lps = [bt.peaked(rs, A, T) for T in T_b]
    K = 4
    hyps, _ = ctc_fast.decode_beam_batch(lps, beam=8, alpha=0.8, beta=0.5, lm=lm, nbest=K)
    ids, lens, _ = ctc_fast.decode_beam_batch(lps, beam=8, alpha=0.8, beta=0.5, lm=lm, nbest=K, device=True)
    base = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    off = [K * int(base[b]) + n * T_b[b] for b in range(3) for n in range(K)]
    flat = [h for row in hyps for h in row]
    assert max(len(h) for h in flat) > 3
    for model in (lm, rnn):
        want = ctc_fast.lm_score_batch(flat, model)
        got = ctc_fast.lm_score_batch((ids, lens, off), model)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, ctc_fast.lm_sentence_scores(flat, model))


# ---- 4. status 2, guard words, the exact workspace ----------------------------------------------------------------

@pytest.mark.parametrize("kind,name", [("rnn", "fix"), ("nn", "fix"), ("ngram", "5g")])
@pytest.mark.parametrize("with_terms", [True, False])
def test_status_2_guards_and_exact_workspace(kind, name, with_terms):
    import torch
    import _sctc
    import ctc_fast
    L = _sctc.lib()
    lm = dev_lm(kind, name)
    rs = np.random.RandomState(3)
    seqs = [rs.randint(1, A, size=u).astype(np.int32) for u in (9, 6, 40, 5, 0, 7, 3)]
    seqs[1][2] = 0              # the blank
    seqs[2][39] = A             # outside the alphabet, and the LM's symbol map
    seqs[5][0] = -7
    seqs[6][1] = 1 << 30
    bad = [1, 2, 5, 6]
    U = np.asarray([len(s) for s in seqs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(U)[:-1]]).astype(np.int64)
    sw = np.ascontiguousarray(lm.sym_words[:A], dtype=np.int32)
    cfg = _sctc.LmScoreConfig(len(seqs), A, {"ngram": 0, "nn": 1, "rnn": 2}[kind], 0, lm.handle, _sctc.i32(sw), _sctc.i32(U),
                              _sctc.i64(off))
    need = ctypes.c_size_t(0)
    _sctc.check(L.sctc_lm_score_workspace_bytes(ctypes.byref(cfg), 0 if with_terms else 1, ctypes.byref(need)), "bytes")
    other = ctypes.c_size_t(0)
    _sctc.check(L.sctc_lm_score_workspace_bytes(ctypes.byref(cfg), 1 if with_terms else 0, ctypes.byref(other)), "bytes")
    pad = (4 * int(U.sum()) + 255) // 256 * 256
    assert (other.value - need.value) == (pad if with_terms else -pad)
    sizes = [need.value, 4 * int(U.sum()), 8 * len(seqs), 4 * len(seqs)]
    offs, pos = [], 256
    for s in sizes:
        offs.append(pos)
        pos = (pos + s + 256 + 255) // 256 * 256
    buf = torch.full((pos,), PATTERN, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 256 == 0
    labels = torch.from_numpy(np.concatenate(seqs)).cuda()
    args = (ctypes.byref(cfg), labels.data_ptr(), base + offs[1] if with_terms else None, base + offs[2], base + offs[3],
            base + offs[0])
    assert L.sctc_lm_score_batch(*args, need.value - 1, _sctc.current_stream_ptr()) == -3      # SCTC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == PATTERN).all()
    _sctc.check(L.sctc_lm_score_batch(*args, need.value, _sctc.current_stream_ptr()), "lm_score")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    inside = np.zeros(pos, dtype=bool)
    for o, s in zip(offs, sizes):
        inside[o:o + s] = True
    assert (out[~inside] == PATTERN).all()
    status = out[offs[3]:offs[3] + sizes[3]].view(np.int32)
    sums = out[offs[2]:offs[2] + sizes[2]].view(np.float64)
    terms = out[offs[1]:offs[1] + sizes[1]]
    assert status.tolist() == [2 if i in bad else 0 for i in range(len(seqs))]
    good = [i for i in range(len(seqs)) if i not in bad]
    want = ctc_fast.lm_sentence_scores([seqs[i] for i in good], lm)
    np.testing.assert_array_equal(sums[good], want)
    assert (sums[bad] == NEG).all()
    for i in range(len(seqs)):
        mine = terms[4 * off[i]:4 * (off[i] + U[i])]
        if i in bad or not with_terms:
            assert (mine == PATTERN).all()          # the terms of a rejected sequence are not written
    if with_terms:
        ht = host_terms(lm, [seqs[i] for i in good])
        for i, t in zip(good, ht):
            np.testing.assert_array_equal(terms[4 * off[i]:4 * (off[i] + U[i])].view(np.float32), t)


def test_empty_batches_launch_nothing():
    import ctc_fast
    lm = dev_lm("ngram", "2g")
    assert ctc_fast.lm_score_batch([], lm).shape == (0,)
    np.testing.assert_array_equal(ctc_fast.lm_score_batch([[], []], dev_lm("rnn", "fix")), [0.0, 0.0])
    with pytest.raises(ValueError):
        ctc_fast.lm_score_batch([[1, 2]], None)
    with pytest.raises(ValueError):
        ctc_fast.lm_score_batch([np.ones(8192, dtype=np.int32)], lm)


# ---- 5. perplexity ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ngram", "nn", "rnn"])
@pytest.mark.parametrize("eos", [True, False])
def test_lm_perplexity(kind, eos):
    import ctc_fast
    base = dev_lm(kind, "2g" if kind == "ngram" else "fix")
    # the LM's own ids under the identity map: a handle of the same model whose symbol c is LM id c
    if kind == "ngram":
        V, end = len(base.arpa.words) + 1, base.arpa.vocab["</s>"]
        ident = ctc_fast.DecodeLM(base.arpa, np.arange(V, dtype=np.int32))
        usable = sorted(set(int(w) for w in base.sym_words[1:]))
    else:
        model = base.nnlm if kind == "nn" else base.rnnlm
        V, end = model.V, model.eos
        ident = (ctc_fast.DecodeNNLM if kind == "nn" else ctc_fast.DecodeRNNLM)(model, np.arange(V, dtype=np.int32))
        usable = sorted(set(int(w) for w in base.sym_words[1:]))
    rs = np.random.RandomState(23)
    text = [[usable[j] for j in rs.randint(0, len(usable), size=u)] for u in (12, 1, 30, 7)]
    rows = [np.asarray(s + ([end] if eos else []), dtype=np.int32) for s in text]
    host = ctc_fast.lm_sentence_scores(rows, ident)          # the sums of the host terms, </s> included
    n = sum(len(r) for r in rows)
    mean = float(np.sum(host)) / n
    pp, bpc, count = ctc_fast.lm_perplexity(text, base, eos=eos)
    assert count == n
    assert pp == 10.0 ** (-mean)
    assert bpc == -mean * np.log2(10.0)
    assert 1.0 < pp < 1e6
    with pytest.raises(ValueError):
        ctc_fast.lm_perplexity([[0, 3]], base)
    ident.close()


def test_lm_perplexity_tool(tmp_path, capsys):
    """tools/lm_perplexity.py: a text of chars.txt tokens -> the figures of ctc_fast.lm_perplexity over its LM ids"""
    import ctc_fast
    from tools import lm_perplexity
    chars = int_char_map()
    rs = np.random.RandomState(4)
    sents = [[chars[int(c)] for c in rs.randint(1, A, size=u)] for u in (9, 14, 3)]
    text = tmp_path / "text.txt"
    text.write_text("".join(" ".join(s) + "\n" for s in sents) + "\n")
    for kind, path in (("ngram", "lm_char_2g.arpa"), ("rnn", "lm_char_rnn.npz")):
        base = dev_lm(kind, "2g" if kind == "ngram" else "fix")
        word = base.arpa.word_id if kind == "ngram" else base.rnnlm.vocab.__getitem__
        want = ctc_fast.lm_perplexity([[word(t) for t in s] for s in sents], base)
        got = lm_perplexity.main(["--text", str(text), "--chars", os.path.join(GOLDEN, "chars.txt"),
                                  "--lm", os.path.join(GOLDEN, path)])
        assert got == want[0]
        assert ("perplexity %.4f, %.4f bits per character, %d terms in 3 sentences" % want) in capsys.readouterr().out
