"""GPU checks of the word LM in the second pass (sctc_nbest_rank_words_batch in csrc/lm_score.hip; ctc_fast.rescore_nbest
and ctc_fast.score_sentences with ``word_lm``).

Yardsticks: tests/word_lm_model.py for the word sums and the rank rule, ``ctc_fast.align_batch`` for log P_ctc,
``ctc_fast.lm_sentence_scores`` for the character LM; for "the word LM changes something" tests/beam_model.py and
tests/align_model.py on the CPU, where the seeds were chosen; for the bg objective tests/lex_beam_model.py."""
import itertools
import os

import numpy as np
import pytest

from tests import align_model, beam_model, lex_beam_model
from tests import word_lm_model as wm
from tests import test_gpu_align as AL
from tests.test_gpu_rescore import ngram, nbest_case
from tests.test_gpu_word_lm_score import lexicon
from tests.test_word_lm_model_cpu import A, GOLDEN, setup

pytestmark = pytest.mark.gpu
NEG = float("-inf")


# ---- 1. values and order against the rank rule ---------------------------------------------------------------------------

def word_case(dtype):
    """nbest_case of tests/test_gpu_rescore.py with hypotheses that hold spaces and lexicon words"""
    chars = setup("bg")[0]
    T_b, K, wide, hyps, first = nbest_case(dtype)
    hyps[0][0] = np.asarray(wm.spell(chars, "a to"), dtype=np.int32)
    hyps[0][2] = np.asarray(wm.spell(chars, "eat zq a"), dtype=np.int32)
    hyps[0][3] = np.asarray(wm.spell(chars, "a to "), dtype=np.int32)
    hyps[2][0] = np.asarray(wm.spell(chars, "an e"), dtype=np.int32)
    hyps[2][1] = np.asarray(wm.spell(chars, "aoe zz"), dtype=np.int32)
    return T_b, K, wide, hyps, first


def expected(view, T_b, K, hyps, K_b, lm, alpha, beta, kind, word_alpha, word_beta, first=None, **flags):
    import ctc_fast
    B = len(T_b)
    _, _, tree, wlm = setup(kind)
    flat = [h for row in hyps for h in row]
    off = np.concatenate([[0], np.cumsum(T_b)])
    import torch
    rows = torch.cat([view[off[b]:off[b + 1]] for b in range(B) for _ in range(K)])
    lens = [T_b[b] for b in range(B) for _ in range(K)]
    _, _, _, total, status = ctc_fast.align_batch(rows, flat, lengths=lens, total=True)
    lmv = ctc_fast.lm_sentence_scores(flat, lm).reshape(B, K) if lm is not None else None
    wsum, wcount, wstatus, _, _ = wm.score_rows(flat, tree, wlm, A, **flags)
    U = np.asarray([len(h) for h in flat]).reshape(B, K)
    return wm.rank(total.reshape(B, K), status.reshape(B, K), lmv, U, K_b, alpha, beta, wsum.reshape(B, K),
                   wcount.reshape(B, K, 2), wstatus.reshape(B, K), word_alpha, word_beta, first=first)


@pytest.mark.parametrize("kind", ["bg", 4])
@pytest.mark.parametrize("with_char_lm", [False, True])
def test_rescore_nbest_with_a_word_lm_against_the_rank_rule(kind, with_char_lm):
    import torch
    import ctc_fast
    lm = ngram() if with_char_lm else None
    alpha, beta, wa, wb = 0.7, 0.4, 1.3, 0.9
    T_b, K, wide, hyps, first = word_case(np.float32)
    K_b = [4, 4, 2]
    dev = torch.from_numpy(wide).cuda()
    view = dev[:, :A]
    lex = lexicon(kind)
    for flags, kw in ((dict(), dict()), (dict(eos=True, final_word=False), dict(word_eos=True, word_final=False))):
        want_order, want = expected(view, T_b, K, hyps, K_b, lm, alpha, beta, kind, wa, wb, **flags)
        assert want[1, 1] == NEG and np.isfinite(want[0]).all() and np.isfinite(want[2, :2]).all()
        order, res = ctc_fast.rescore_nbest(view, hyps, lengths=T_b, lm=lm, alpha=alpha, beta=beta, K_b=K_b, word_lm=lex,
                                            word_alpha=wa, word_beta=wb, **kw)
        assert order.dtype == np.int32 and res.dtype == np.float64
        np.testing.assert_array_equal(res, want)
        np.testing.assert_array_equal(order, want_order)
        # the device route: the tensors as a search leaves them; the ranks beyond the beam told by the first scores
        ids = np.zeros(K * sum(T_b), dtype=np.int32)
        base = np.concatenate([[0], np.cumsum(T_b)])
        for b in range(3):
            for n in range(K):
                o = K * base[b] + n * T_b[b]
                ids[o:o + len(hyps[b][n])] = hyps[b][n]
        lens = np.asarray([len(h) for row in hyps for h in row], dtype=np.int32)
        triple = (torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(first.reshape(-1)).cuda())
        d_order, d_res = ctc_fast.rescore_nbest(view, triple, lengths=T_b, lm=lm, alpha=alpha, beta=beta, device=True,
                                                word_lm=lex, word_alpha=wa, word_beta=wb, **kw)
        assert d_order.is_cuda and d_res.is_cuda
        w_order, w_res = expected(view, T_b, K, hyps, [K] * 3, lm, alpha, beta, kind, wa, wb, first=first, **flags)
        np.testing.assert_array_equal(d_res.cpu().numpy(), w_res)
        np.testing.assert_array_equal(d_order.cpu().numpy(), w_order)
        np.testing.assert_array_equal(w_res, want)


@pytest.mark.parametrize("with_char_lm", [False, True])
def test_zero_word_weights_give_the_rescoring_without_a_word_lm(with_char_lm):
    import ctc_fast
    lm = ngram() if with_char_lm else None
    T_b, K, wide, hyps, first = word_case(np.float64)
    lps = [np.ascontiguousarray(wide[o:o + t, :A].T) for o, t in zip(np.concatenate([[0], np.cumsum(T_b)]), T_b)]
    plain = ctc_fast.rescore_nbest(lps, hyps, lm=lm, alpha=0.7, beta=0.4, scores=first)
    zero = ctc_fast.rescore_nbest(lps, hyps, lm=lm, alpha=0.7, beta=0.4, scores=first, word_lm=lexicon("bg"),
                                  word_alpha=0.0, word_beta=0.0)
    assert zero[1].tobytes() == plain[1].tobytes() and zero[0].tobytes() == plain[0].tobytes()
    assert np.isfinite(plain[1]).sum() >= 9


def test_a_hypothesis_the_word_lm_cannot_score_is_minus_infinity(tmp_path):
    import ctc_fast
    from decoder import lm as lm_mod, prefixTree
    chars = setup("bg")[0]
    path = tmp_path / "no_unk.arpa"
    path.write_text("\\data\\\nngram 1=4\nngram 2=1\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-0.7\ta\t-0.3\n"
                    "-0.9\teat\t-0.2\n\n\\2-grams:\n-0.4\ta eat\n\n\\end\\\n")
    lm = lm_mod.LM(str(path))
    lex = ctc_fast.DecodeLexicon.from_tree(prefixTree.PrefixTree(chars, ["a", "eat"], lm), lm, A)
    rs = np.random.RandomState(3)
    lps = [AL.rand_y(rs, A, 12)]
    hyps = [[np.asarray(wm.spell(chars, t), dtype=np.int32) for t in ("a to", "a eat", "eat")]]
    order, res = ctc_fast.rescore_nbest(lps, hyps, word_lm=lex, word_alpha=0.0, word_beta=0.0)
    assert res[0, 0] == NEG and np.isfinite(res[0, 1:]).all() and order[0, 2] == 0 and not np.isnan(res).any()
    sent = ctc_fast.score_sentences(lps * 3, hyps[0], word_lm=lex, word_alpha=0.0)
    assert sent[0] == NEG and sent[1:].tobytes() == res[0, 1:].tobytes()
    lex.close()


# ---- 2. the word LM changes the 1-best ----------------------------------------------------------------------------------

SEEDS = (0, 1, 2, 3, 4, 5)
N_CHANGED = 2                   # seeds 2 and 5: counted on the CPU with the host models below (model_picks)
KBEST = 6
WORD = dict(word_alpha=0.6, word_beta=0.5)
PICK_MARGIN = 1e-6              # far above the 1e-11 relative error of log P_ctc, far below the gaps that decide


def noisy_sentence(seed):
    """log-probabilities that spell a sentence of lexicon words, one frame a symbol, loudly enough for the sentence to
    be in the beam and not loudly enough to be its 1-best everywhere"""
    chars, words, _, _ = setup("bg")
    rs = np.random.RandomState(100 + seed)
    short = [w for w in words[:60] if len(w) <= 4]
    path = []
    for c in wm.spell(chars, " ".join(short[rs.randint(len(short))] for _ in range(4))):
        if path and path[-1] == c:
            path.append(0)
        path.append(c)
    z = rs.randn(A, len(path)) * 1.2
    for t, c in enumerate(path):
        z[c, t] += 3.0
    return np.asfortranarray(AL.log_softmax_cols(z))


def model_picks():
    """on the CPU: the lexicon-free first pass's K best (tests/beam_model.py, no LM) and each one's second-pass score
    from tests/align_model.py and tests/word_lm_model.py -> [(logprobs, hyps, scores, pick, margin)]"""
    _, _, tree, lm = setup("bg")
    out = []
    for seed in SEEDS:
        lp = noisy_sentence(seed)
        best = beam_model.decode(lp, 12, 0.0, 0.0, None, nbest=KBEST)
        hyps = [np.asarray(P, dtype=np.int32) for P, _ in best]
        scores = []
        for h in hyps:
            with np.errstate(all="ignore"):
                total = align_model.align(lp, h, total=True).total
            w = wm.score_row(h, tree, lm, A)
            scores.append(wm.combine(total, 0.0, len(h), 0.0, 0.0, w["sum"], w["words"], w["status"],
                                     WORD["word_alpha"], WORD["word_beta"]))
        scores = np.asarray(scores)
        k = int(np.argmax(scores))
        out.append((lp, hyps, scores, k, scores[k] - np.max(np.delete(scores, k))))
    return out


def test_the_word_lm_changes_the_one_best():
    import ctc_fast
    cases = model_picks()
    assert all(len(h) == KBEST for _, h, _, _, _ in cases)
    changed = [i for i, c in enumerate(cases) if c[3] != 0 and c[4] > PICK_MARGIN]
    for seed, c in zip(SEEDS, cases):
        print("seed %d: model picks rank %d, margin %.3g" % (seed, c[3], c[4]))
    assert len(changed) == N_CHANGED >= 1
    order, res = ctc_fast.rescore_nbest([c[0] for c in cases], [c[1] for c in cases], lm=None, alpha=0.0, beta=0.0,
                                        word_lm=lexicon("bg"), **WORD)
    assert sum(int(o[0]) != 0 for o in order) >= N_CHANGED
    for i, c in enumerate(cases):
        if c[4] > PICK_MARGIN:
            assert order[i, 0] == c[3], (SEEDS[i], order[i], c[3])
        assert np.abs(res[i] - c[2]).max() <= 1e-9 * np.abs(c[2]).max()


# ---- 3. the bg search against score_sentences ---------------------------------------------------------------------------

BG_WORDS = ["a", "e", "ae", "ee", "eaa", "aaa"]
BG_GAP_MEASURED = 5.9e-08       # bg_search_gap_on_the_host() gives 5.872e-08: float32 masses between frames
BG_MARGIN = 4 * BG_GAP_MEASURED


def bg_objects():
    from decoder import lm as lm_mod, prefixTree
    lm = lm_mod.LM(os.path.join(GOLDEN, "lm_word_2g.arpa"))
    chars = {tok: sym for sym, tok in AL.SEARCH_SYMBOLS.items()}
    return prefixTree.PrefixTree(chars, BG_WORDS, lm), lm


def spelled(tree, sentence):
    """a prefix the lexicon search can hold: a space only after a word, letters only along the tree"""
    toks = wm.tokens_of(sentence, tree.space)
    if len(sentence) - sum(len(t) for t, _ in toks) != sum(1 for _, spaced in toks if spaced):
        return False                                    # a leading or a repeated space
    for tok, spaced in toks:
        node, steps = wm.walk(tree, tok)
        if node is None or (spaced and not node.isWord):
            return False
    return True


def host_bg_score(y, l, tree, lm, alpha, beta):
    with np.errstate(all="ignore"):
        total = align_model.align(y, l, total=True).total
    w = wm.score_row(l, tree, lm, 4, final_word=False)
    return wm.combine(total, 0.0, len(l), 0.0, 0.0, w["sum"], w["words"], w["status"], alpha, beta)


def bg_search_gap_on_the_host():
    """worst |tests/lex_beam_model.py top score - float64 model score of that hypothesis| over the test's inputs"""
    tree, lm = bg_objects()
    args = lex_beam_model.from_objects(tree, lm, 4)
    worst = 0.0
    for y in AL.search_inputs():
        (hyp, score), = lex_beam_model.decode(y, *args, beam=AL.SEARCH_BEAM, alpha=AL.SEARCH_ALPHA, beta=AL.SEARCH_BETA)
        worst = max(worst, abs(score - host_bg_score(y, list(hyp), tree, lm, AL.SEARCH_ALPHA, AL.SEARCH_BETA)))
    return worst


def test_bg_search_against_score_sentences():
    """With a beam that holds every lexicon-consistent prefix (at most 121 strings of 4 symbols out of 3, beam 128) the
    word search's top score is the sentence score of its hypothesis under ``score_sentences(word_lm=..., word_final=
    False)``, up to the float32 rounding of the beam's masses between frames: the gap measured on the CPU between
    tests/lex_beam_model.py and the float64 model over these inputs is asserted, the test allows 4 x it.  No other
    spelled sentence scores higher than the top by more than that margin."""
    import ctc_fast
    tree, lm = bg_objects()
    ys = AL.search_inputs()
    assert bg_search_gap_on_the_host() <= BG_GAP_MEASURED
    sentences = [list(r) for n in range(5) for r in itertools.product((1, 2, 3), repeat=n)]
    consistent = [s for s in sentences if spelled(tree, s)]
    assert len(sentences) == 121 <= AL.SEARCH_BEAM and 30 <= len(consistent) < 121
    lex = ctc_fast.DecodeLexicon.from_tree(tree, lm, 4)
    try:
        hyps, scores = ctc_fast.decode_lexicon_beam_batch(ys, lexicon=lex, beam=AL.SEARCH_BEAM, alpha=AL.SEARCH_ALPHA,
                                                          beta=AL.SEARCH_BETA)
        kw = dict(word_lm=lex, word_alpha=AL.SEARCH_ALPHA, word_beta=AL.SEARCH_BETA, word_final=False)
        own = ctc_fast.score_sentences(ys, hyps, **kw)
        assert np.all(np.abs(own - scores) <= BG_MARGIN), (own, scores)
        assert sum(1 for h in hyps if 1 in h.tolist()) > 0            # some hypotheses finish a word
        for b, y in enumerate(ys):
            every = ctc_fast.score_sentences([y] * len(consistent), consistent, **kw)
            assert every.max() <= scores[b] + BG_MARGIN, (b, every.max(), scores[b])
            want = host_bg_score(y, consistent[5], tree, lm, AL.SEARCH_ALPHA, AL.SEARCH_BETA)
            assert every[5] == want or abs(every[5] - want) <= AL.TOTAL_RTOL * abs(want)
    finally:
        lex.close()


# ---- 4. the driver ------------------------------------------------------------------------------------------------------

from tests.test_gpu_rescore import shard_likelihoods  # noqa: E402,F401  (the fixture)


def test_run_decode_rescore_word_lm_on_the_golden_shard(shard_likelihoods, tmp_path, capsys):  # noqa: F811
    import pickle
    import ctc_fast
    import runDecode
    from new_decoder import decoder
    chars = os.path.join(GOLDEN, "chars.txt")
    lm2 = os.path.join(GOLDEN, "lm_char_2g.arpa")
    wlm = os.path.join(GOLDEN, "lm_word_4g.arpa")
    wlist = os.path.join(GOLDEN, "words_bg.txt")
    common = ["--likelihoods", shard_likelihoods, "--chars", chars, "--alis", os.path.join(GOLDEN, "shard", "alis1.txt"),
              "--lm", lm2, "--beam", "8", "--alpha", "0.5", "--beta", "0.3", "--batch", "3"]
    word = ["--rescore-word-lm", wlm, "--rescore-words", wlist, "--rescore-word-lm-order", "3", "--rescore-word-alpha", "0.8",
            "--rescore-word-beta", "0.4"]
    with open(shard_likelihoods, "rb") as f:
        pk = pickle.load(f)
    keys = sorted(pk)
    d = decoder.BeamLMDecoder()
    d.load_chars(chars)
    d.load_lm(lm2)
    lex = ctc_fast.DecodeLexicon(wlist, d.char_int_map, wlm, "[space]", A=A, order=3)
    for extra, kw in (([], dict()), (["--rescore-lm", lm2, "--rescore-alpha", "1.5"], dict(rescore_lm=lm2, rescore_alpha=1.5))):
        resc = tmp_path / "rescored.txt"
        cer = runDecode.main(common + ["--out", str(resc), "--rescore-nbest", "4"] + word + extra)
        said = capsys.readouterr().out
        line = [l for l in said.splitlines() if l.startswith("rescored: ")]
        assert len(line) == 1 and line[0].endswith("of %d utterances changed their 1-best" % len(keys))
        assert np.isfinite(cer) and cer >= 0
        got = resc.read_text().splitlines()
        assert len(got) == len(keys)
        changed = 0
        for g in range(0, len(keys), 3):
            ks = keys[g:g + 3]
            probs = [np.asfortranarray(pk[k], dtype=np.float64) for k in ks]
            first = d.decode_batch(probs, 8, 0.5, 0.3, nbest=4)
            second = d.decode_batch(probs, 8, 0.5, 0.3, nbest=4, rescore_word_lm=lex, rescore_word_alpha=0.8,
                                    rescore_word_beta=0.4, **kw)
            changed += sum(d.rescore_changed)
            for k, f_row, s_row in zip(ks, first, second):
                assert got[keys.index(k)] == "%s %.6f %s" % (k, s_row[0][1], s_row[0][0])
                assert sorted(h for h, _ in f_row) == sorted(h for h, _ in s_row)
                vals = [s for _, s in s_row if s > NEG]
                assert vals == sorted(vals, reverse=True)
        assert line[0].startswith("rescored: %d of" % changed)
    lex.close()
    with pytest.raises(SystemExit):
        runDecode.main(common + ["--out", str(resc)] + word)                                     # no --rescore-nbest
    with pytest.raises(SystemExit):
        runDecode.main(common + ["--out", str(resc), "--rescore-nbest", "4", "--rescore-word-lm", wlm])     # no word list


def test_run_decode_bg_ref_scores(shard_likelihoods, tmp_path, capsys):  # noqa: F811
    import pickle
    import ctc_fast
    import runDecode
    from decoder import decoder_utils
    chars = os.path.join(GOLDEN, "chars.txt")
    wlm = os.path.join(GOLDEN, "lm_word_2g.arpa")
    wlist = os.path.join(GOLDEN, "words_bg.txt")
    alis = os.path.join(GOLDEN, "shard", "alis1.txt")
    out, ref = tmp_path / "hyp.txt", tmp_path / "ref.txt"
    runDecode.main(["--method", "bg", "--likelihoods", shard_likelihoods, "--chars", chars, "--alis", alis, "--words", wlist,
                    "--word-lm", wlm, "--specials", "[laughter]", "[noise]", "--out", str(out), "--beam", "8",
                    "--alpha", "0.8", "--beta", "0.37", "--batch", "3", "--ref-scores", str(ref)])
    assert "ref scores of" in capsys.readouterr().out
    with open(shard_likelihoods, "rb") as f:
        pk = pickle.load(f)
    cmap = decoder_utils.load_chars(chars)
    refs = runDecode.load_alis(alis, chars)
    keys = [k for k in sorted(pk) if k in refs]
    lex = ctc_fast.DecodeLexicon(wlist, cmap, wlm, "[space]", specials=["[laughter]", "[noise]"])
    want = ctc_fast.score_sentences([np.asarray(pk[k]) for k in keys], [[cmap.get(t, -1) for t in refs[k]] for k in keys],
                                    word_lm=lex, word_alpha=0.8, word_beta=0.37, word_final=False)
    hyp = {l.split()[0]: l.split()[1] for l in out.read_text().splitlines()}
    lines = ref.read_text().splitlines()
    assert len(lines) == len(keys) >= 1
    for line, k, w in zip(lines, keys, want):
        key, hs, rs = line.split()
        assert key == k and hs == hyp[k] and float(rs) == float("%.6f" % w)
    lex.close()
