"""GPU checks of n-best rescoring (nbest_rank_kernel in csrc/lm_score.hip; ctc_fast.rescore_nbest).

Yardsticks: ``ctc_fast.score_sentences`` (untouched: one align launch and the host LM route) for the value of every
real hypothesis, equal bits; tests/rescore_model.py for the order; and for "rescoring does something" the float64
models -- tests/beam_model.py with the 2-gram for the first pass, tests/align_model.py for log P_ctc and
tests/rnn_lm_model.py (rows64) for the recurrent LM -- evaluated on the CPU, where the seeds were chosen."""
import os

import numpy as np
import pytest

from tests import align_model, beam_model, rescore_model
from tests import beam_trace as bt
from tests import rnn_lm_model
from tests.beam_harness import int_char_map
from tests import test_gpu_decode_rnn as RNN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEG = float("-inf")
A = 35
_LM = {}


def ngram():
    import ctc_fast
    if "2g" not in _LM:
        _LM["2g"] = ctc_fast.DecodeLM(os.path.join(GOLDEN, "lm_char_2g.arpa"), int_char_map(), A)
    return _LM["2g"]


# ---- 1. values against score_sentences, order against the model -----------------------------------------------------

def nbest_case(dtype):
    """B = 3, K = 4 over a tensor with ld = 48 > A: utterance 1 holds a hypothesis that cannot be aligned (three
    repeats need 7 frames of its 5), utterance 2 has two real hypotheses (the first pass left ranks 2, 3 at -inf)"""
    rs = np.random.RandomState(31)
    T_b = [12, 5, 9]
    K = 4
    wide = np.full((sum(T_b), 48), 7.0, dtype=dtype)          # the columns beyond A are never read
    lps = [bt.peaked(rs, A, T) for T in T_b]
    wide[:, :A] = np.concatenate([lp.T for lp in lps], axis=0)
    hyps = [[rs.randint(1, A, size=u).astype(np.int32) for u in (4, 0, 7, 3)],
            [np.asarray(h, dtype=np.int32) for h in ([5], [3, 3, 3, 3], [9, 2], [])],
            [rs.randint(1, A, size=u).astype(np.int32) for u in (5, 6)] + [np.zeros(0, np.int32)] * 2]
    hyps[0][3] = hyps[0][0][:3].copy()
    first = np.array([[-1.0, -2.0, -3.0, -4.0], [-1.0, -1.5, -2.5, -3.0], [-2.0, -2.5, NEG, NEG]])
    return T_b, K, wide, hyps, first


def expected(wide_dev, T_b, K, hyps, K_b, lm, alpha, beta):
    """score_sentences over the B * K pairs (every hypothesis with a copy of its utterance's rows), -inf where the rank
    is no hypothesis; the order by tests/rescore_model.py from the host route's own parts"""
    import torch
    import ctc_fast
    off = np.concatenate([[0], np.cumsum(T_b)])
    rows = torch.cat([wide_dev[off[b]:off[b + 1]] for b in range(len(T_b)) for _ in range(K)])[:, :A]
    assert rows.stride(0) > A
    flat = [h for row in hyps for h in row]
    lens = [T_b[b] for b in range(len(T_b)) for _ in range(K)]
    want = ctc_fast.score_sentences(rows, flat, lengths=lens, lm=lm, alpha=alpha, beta=beta).reshape(len(T_b), K)
    _, _, _, total, status = ctc_fast.align_batch(rows, flat, lengths=lens, total=True)
    lmv = ctc_fast.lm_sentence_scores([h if s == 0 else h[:0] for h, s in zip(flat, status)], lm) if lm is not None else None
    U = np.asarray([len(h) for h in flat]).reshape(len(T_b), K)
    order, model = rescore_model.rank(total.reshape(-1, K), status.reshape(-1, K),
                                      None if lmv is None else lmv.reshape(-1, K), U, K_b, alpha, beta)
    for b in range(len(T_b)):
        want[b, K_b[b]:] = NEG
    np.testing.assert_array_equal(model, want)              # the model is score_sentences' operation order
    return want, order, status.reshape(-1, K)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lm_name", ["rnn", "2g", None])
def test_rescore_nbest_against_score_sentences(dtype, lm_name):
    import torch
    import ctc_fast
    lm = {"rnn": lambda: RNN.dev_lm("fix", A), "2g": ngram, None: lambda: None}[lm_name]()
    alpha, beta = 0.7, 0.4
    T_b, K, wide, hyps, first = nbest_case(dtype)
    K_b = [4, 4, 2]
    dev = torch.from_numpy(wide).cuda()
    view = dev[:, :A]
    want, want_order, status = expected(dev, T_b, K, hyps, K_b, lm, alpha, beta)
    assert status[1, 1] == 1 and want[1, 1] == NEG and (status[np.isfinite(want)] == 0).all()
    assert np.isfinite(want[0]).all() and np.isfinite(want[2, :2]).all()
    # the list route, the ranks beyond the beam told by K_b, then by the first pass's scores
    for kw in (dict(K_b=K_b), dict(scores=first)):
        order, res = ctc_fast.rescore_nbest(view, hyps, lengths=T_b, lm=lm, alpha=alpha, beta=beta, **kw)
        assert order.dtype == np.int32 and res.dtype == np.float64 and order.shape == res.shape == (3, K)
        np.testing.assert_array_equal(res, want)
        np.testing.assert_array_equal(order, want_order)
    assert order[2].tolist()[2:] == [2, 3] and order[1].tolist()[3] == 1
    # the device route: the tensors as a search leaves them (rank n of utterance b from K * sum T_<b + n * T_b)
    ids = np.zeros(K * sum(T_b), dtype=np.int32)
    base = np.concatenate([[0], np.cumsum(T_b)])
    for b in range(3):
        for n in range(K):
            o = K * base[b] + n * T_b[b]
            ids[o:o + len(hyps[b][n])] = hyps[b][n]
    lens = np.asarray([len(h) for row in hyps for h in row], dtype=np.int32)
    triple = (torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(first.reshape(-1)).cuda())
    d_order, d_res = ctc_fast.rescore_nbest(view, triple, lengths=T_b, lm=lm, alpha=alpha, beta=beta, device=True)
    assert d_order.is_cuda and d_res.is_cuda
    np.testing.assert_array_equal(d_res.cpu().numpy(), want)
    np.testing.assert_array_equal(d_order.cpu().numpy(), want_order)
    # host arrays in, (A, T) per utterance as the decoders take them
    lps = [np.ascontiguousarray(wide[base[b]:base[b + 1], :A].T) for b in range(3)]
    order, res = ctc_fast.rescore_nbest(lps, hyps, lm=lm, alpha=alpha, beta=beta, K_b=K_b)
    np.testing.assert_array_equal(res, want)
    np.testing.assert_array_equal(order, want_order)


def test_ties_and_no_real_hypotheses():
    """equal hypotheses tie exactly: the lower first-pass rank goes first; K_b = 0 keeps the original order"""
    import ctc_fast
    rs = np.random.RandomState(2)
    lps = [bt.peaked(rs, A, 10), bt.peaked(rs, A, 8)]
    h = rs.randint(1, A, size=3).astype(np.int32)
    g = rs.randint(1, A, size=2).astype(np.int32)
    hyps = [[g, h, h.copy(), h.copy()], [h, g, g, h]]
    order, res = ctc_fast.rescore_nbest(lps, hyps, lm=ngram(), alpha=1.0, beta=0.0, K_b=[4, 0])
    assert res[0, 1] == res[0, 2] == res[0, 3] and np.isfinite(res[0]).all()
    assert order[0].tolist() == ([1, 2, 3, 0] if res[0, 1] > res[0, 0] else [0, 1, 2, 3])
    assert order[1].tolist() == [0, 1, 2, 3] and (res[1] == NEG).all()


# ---- 2. rescoring does something --------------------------------------------------------------------------------------

SEEDS = (0, 3, 5, 7)                  # chosen on the CPU: SEEDS_THAT_CHANGE of them meet both conditions; at seed 7 the
SEEDS_THAT_CHANGE = (0, 3, 5)         # recurrent LM agrees with the first pass, by a margin beyond the bound too
FIRST = dict(beam=12, alpha=0.5, beta=0.5)
SECOND = dict(alpha=2.0, beta=0.5)
KBEST, FRAMES = 6, 40


def model_rescoring(seed):
    """on the CPU, in float64: the first pass's K best under the 2-gram, and each one's second-pass score under the
    recurrent LM fixture -> (logprobs, hypotheses, float64 scores)"""
    import arpa_lm
    lp = bt.peaked(np.random.RandomState(seed), A, FRAMES)
    arpa = arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_2g.arpa"))
    sw2 = arpa.symbol_words(int_char_map(), A)
    best = beam_model.decode(lp, FIRST["beam"], FIRST["alpha"], FIRST["beta"], beam_model.arpa_rows(arpa, sw2), nbest=KBEST)
    hyps = [np.asarray(P, dtype=np.int32) for P, _ in best]
    row = rnn_lm_model.rows64(RNN.host_lm("fix"), RNN.sym_words("fix", A))
    scores = []
    for h in hyps:
        total = align_model.align(lp, h, total=True).total
        lm = sum(float(row(tuple(h[:i]))[int(c)]) for i, c in enumerate(h))
        scores.append((total + SECOND["alpha"] * lm) + SECOND["beta"] * len(h))
    return lp, hyps, np.asarray(scores)


def decided(hyps, scores, d32):
    """the conditions of the test: the best under the recurrent LM is not rank 0, and it leads every other hypothesis
    by more than 2 * d32 * alpha * (U + 1), U the longest hypothesis: the float32 rows cannot change the pick"""
    k = int(np.argmax(scores))
    margin = scores[k] - np.max(np.delete(scores, k))
    bound = 2.0 * d32 * SECOND["alpha"] * (max(len(h) for h in hyps) + 1)
    return k, margin, bound, (k != 0 and margin > bound)


def test_rescoring_changes_the_one_best():
    import ctc_fast
    d32 = RNN.yardstick("fix")[4]
    cases = [model_rescoring(seed) for seed in SEEDS]
    picks = [decided(h, s, d32) for _, h, s in cases]
    changed = [i for i, p in enumerate(picks) if p[3]]
    for seed, p in zip(SEEDS, picks):
        print("seed %d: model picks rank %d, margin %.3g, bound %.3g%s" % (seed, p[0], p[1], p[2], " *" if p[3] else ""))
    assert changed, "no seed meets the model conditions: the test would pass vacuously"
    assert [SEEDS[i] for i in changed] == list(SEEDS_THAT_CHANGE)
    assert all(len(h) == KBEST for _, h, _ in cases)
    order, res = ctc_fast.rescore_nbest([lp for lp, _, _ in cases], [h for _, h, _ in cases], lm=RNN.dev_lm("fix", A),
                                        **SECOND)
    for i in changed:
        assert order[i, 0] == picks[i][0] != 0, (SEEDS[i], order[i], picks[i])
    for i, p in enumerate(picks):                # wherever the margin decides, the device agrees with the model
        if p[1] > p[2]:
            assert order[i, 0] == p[0], (SEEDS[i], order[i], p)
    for i, (_, h, s) in enumerate(cases):        # and every value is the model's, to the rows' float32 error
        assert np.abs(res[i] - s).max() <= picks[i][2]


# ---- 3. the decoder and the driver ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shard_likelihoods(tmp_path_factory):
    """the golden shard through a small BRNN: the pickle that runDecode.py reads"""
    import dataLoader as dl
    import writeLikelihoods as wl
    from nnets import brnnet
    g = np.load(os.path.join(GOLDEN, "loader_ref.npz"))
    raw = int(g["rawsize"])
    net = brnnet.NNet(raw, A, 32, 3, 200, train=False, temporalLayer=2)
    np.random.seed(1)
    net.initParams()
    loader = dl.DataLoader(os.path.join(GOLDEN, "shard") + "/", raw, raw)
    lik = tmp_path_factory.mktemp("lik")
    wl.writeLogLikes(loader, net, 1, str(lik), writePickle=True)
    return str(lik / "loglikelihoods_1.pk")


def test_run_decode_rescore_lm_on_the_golden_shard(shard_likelihoods, tmp_path, capsys):
    import pickle
    import runDecode
    from new_decoder import decoder
    chars = os.path.join(GOLDEN, "chars.txt")
    lm2 = os.path.join(GOLDEN, "lm_char_2g.arpa")
    rnn = os.path.join(GOLDEN, "lm_char_rnn.npz")
    common = ["--likelihoods", shard_likelihoods, "--chars", chars, "--alis", os.path.join(GOLDEN, "shard", "alis1.txt"),
              "--lm", lm2, "--beam", "8", "--alpha", "0.5", "--beta", "0.3", "--batch", "3"]
    plain, resc = tmp_path / "plain.txt", tmp_path / "rescored.txt"
    runDecode.main(common + ["--out", str(plain)])
    assert "rescored:" not in capsys.readouterr().out
    # without the flag: byte for byte what the decoder's first pass alone writes
    with open(shard_likelihoods, "rb") as f:
        pk = pickle.load(f)
    d = decoder.BeamLMDecoder()
    d.load_chars(chars)
    d.load_lm(lm2)
    keys = sorted(pk)
    want = ""
    for g in range(0, len(keys), 3):
        ks = keys[g:g + 3]
        probs = [np.asfortranarray(pk[k], dtype=np.float64) for k in ks]
        for k, (hyp, score) in zip(ks, d.decode_batch(probs, 8, 0.5, 0.3)):
            want += "%s %.6f %s\n" % (k, score, hyp)
    assert plain.read_bytes() == want.encode()
    # with it: it runs, says so, and every line is the decoder's re-ranked 1-best
    cer = runDecode.main(common + ["--out", str(resc), "--rescore-lm", rnn, "--rescore-nbest", "4", "--rescore-alpha", "1.5"])
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
        second = d.decode_batch(probs, 8, 0.5, 0.3, nbest=4, rescore_lm=rnn, rescore_alpha=1.5)
        changed += sum(d.rescore_changed)
        for k, f_row, s_row in zip(ks, first, second):
            assert got[keys.index(k)] == "%s %.6f %s" % (k, s_row[0][1], s_row[0][0])
            assert sorted(h for h, _ in f_row) == sorted(h for h, _ in s_row)       # a permutation of the first pass
            vals = [s for _, s in s_row if s > NEG]
            assert vals == sorted(vals, reverse=True)
    assert line[0].startswith("rescored: %d of" % changed)
    with pytest.raises(SystemExit):
        runDecode.main(common + ["--out", str(resc), "--rescore-lm", rnn])          # no --rescore-nbest
    with pytest.raises(SystemExit):
        runDecode.main(common + ["--out", str(resc), "--rescore-lm", rnn, "--rescore-nbest", "9"])      # K > beam
