"""GPU checks of the prefix beam search decoder (csrc/ctc_beam.hip): the
reference's own results (tests/golden/decode_ref.npz), the Python restatement
(tests/beam_model.py) at long T and at the limits, batch independence, input types, -inf
input, T = 0 / 1, rejected limits, and runDecode.py on a shard written by writeLikelihoods."""
import os
import pickle

import numpy as np
import pytest

from tests import beam_model
from tests.beam_trace import logsoftmax, peaked
from tests.test_dataloader import write_shard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHARS = os.path.join(GOLDEN, "chars.txt")


def lm_path(k):
    return os.path.join(GOLDEN, "lm_char_%s.arpa" % k)


def beam_decoder(k):
    from new_decoder import decoder
    d = decoder.BeamLMDecoder()
    d.load_chars(CHARS)
    d.load_lm(lm_path(k))
    return d


def assert_same(got_hyp, got_score, ref_hyp, ref_score, margin, what=""):
    assert abs(got_score - ref_score) <= 1e-6 * abs(ref_score) + 1e-9, (what, got_score, ref_score)
    if margin >= 1e-6:
        assert list(got_hyp) == list(ref_hyp), what


def test_against_reference_golden():
    import ctc_fast
    z = np.load(os.path.join(GOLDEN, "decode_ref.npz"))
    decs = {k: beam_decoder(k) for k in ("2g", "5g")}
    lms = {}
    for i in range(int(z["n"])):
        A, T, beam, alpha, beta = z["cfg%d" % i]
        A, T, beam = int(A), int(T), int(beam)
        k = str(z["lm%d" % i])
        lp = z["lp%d" % i]
        d = decs[k]
        hyp, score = d.decode(np.asfortranarray(lp), beam, alpha, beta)
        ref_ids = z["hyp%d" % i]
        assert abs(score - float(z["score%d" % i])) <= 1e-6 * abs(float(z["score%d" % i])), (i, score)
        if z["margin%d" % i] >= 1e-6:
            assert hyp == str(z["hyps%d" % i]), (i, hyp, str(z["hyps%d" % i]))
        # the batched entry with the device LM, float32 device copy of the same data in float64
        if (k, A) not in lms:
            lms[(k, A)] = ctc_fast.DecodeLM(d.lm, d.int_char_map, A)
        hyps, scores = ctc_fast.decode_beam_batch([lp], beam=beam, alpha=alpha, beta=beta, lm=lms[(k, A)])
        assert_same(hyps[0], scores[0], ref_ids, float(z["score%d" % i]), float(z["margin%d" % i]), i)


@pytest.mark.parametrize("T,beam,lm", [(2000, 16, "5g"), (1200, 40, "2g"), (600, 40, None)])
def test_against_restatement_long(T, beam, lm):
    import arpa_lm
    import ctc_fast
    rs = np.random.RandomState(T + beam)
    A = 35
    lp = peaked(rs, A, T)
    rows = None
    dlm = None
    if lm:
        d = beam_decoder(lm)
        alm = arpa_lm.ArpaLM(lm_path(lm))
        dlm = ctc_fast.DecodeLM(alm, d.int_char_map, A)
        rows = beam_model.arpa_rows(alm, dlm.sym_words)
    top = beam_model.decode(lp, beam, 0.8, 0.5, rows, nbest=2)
    hyps, scores = ctc_fast.decode_beam_batch([lp], beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=2)
    margin = top[0][1] - top[1][1]
    assert_same(hyps[0][0], scores[0, 0], top[0][0], top[0][1], margin, "top")
    assert abs(scores[0, 1] - top[1][1]) <= 1e-6 * abs(top[1][1])
    assert len(hyps[0][0]) > T // 10


def test_limits_beam256_a256():
    import ctc_fast
    rs = np.random.RandomState(256)
    A, T = 256, 10
    lp = logsoftmax(3.0 * rs.randn(A, T))
    top = beam_model.decode(lp, 256, 0.0, 0.3, None, nbest=3)
    hyps, scores = ctc_fast.decode_beam_batch([lp, lp[:, :4]], beam=256, alpha=0.0, beta=0.3, nbest=3)
    for n in range(3):
        assert abs(scores[0, n] - top[n][1]) <= 1e-6 * abs(top[n][1]) + 1e-9
    assert_same(hyps[0][0], scores[0, 0], top[0][0], top[0][1], top[0][1] - top[1][1])
    top4 = beam_model.decode(lp[:, :4], 256, 0.0, 0.3, None)
    assert_same(hyps[1][0], scores[1, 0], top4[0][0], top4[0][1], 1.0)
    assert max(int(h.max()) for h in hyps[0] if len(h)) < A


def test_batch_composition_and_order():
    import ctc_fast
    rs = np.random.RandomState(11)
    A = 33
    d = beam_decoder("5g")
    lm = ctc_fast.DecodeLM(d.lm, d.int_char_map, A)
    utts = [peaked(rs, A, T) for T in (50, 1, 120, 0, 77, 200)]
    singles = [ctc_fast.decode_beam_batch([u], beam=24, alpha=1.0, beta=0.5, lm=lm) for u in utts]
    hyps, scores = ctc_fast.decode_beam_batch(utts, beam=24, alpha=1.0, beta=0.5, lm=lm)
    rh, rsc = ctc_fast.decode_beam_batch(utts[::-1], beam=24, alpha=1.0, beta=0.5, lm=lm)
    for b, (sh, ss) in enumerate(singles):
        assert list(hyps[b]) == list(sh[0]) and scores[b] == ss[0]
        assert list(rh[len(utts) - 1 - b]) == list(sh[0]) and rsc[len(utts) - 1 - b] == ss[0]
    # the reference surface's batch form agrees with its single form
    res = d.decode_batch([np.asfortranarray(u) for u in utts], 24, 1.0, 0.5)
    for (h, s), u in zip(res, utts):
        assert (h, s) == d.decode(np.asfortranarray(u), 24, 1.0, 0.5)


def test_float32_and_float64_device_input():
    import torch
    import ctc_fast
    rs = np.random.RandomState(5)
    A = 35
    utts = [peaked(rs, A, T).astype(np.float32) for T in (90, 40, 130)]
    lengths = [u.shape[1] for u in utts]
    rows = np.concatenate([u.T for u in utts], axis=0)
    d = beam_decoder("2g")
    lm = ctc_fast.DecodeLM(d.lm, d.int_char_map, A)
    h32, s32 = ctc_fast.decode_beam_batch(torch.from_numpy(rows).cuda(), lengths, beam=32, lm=lm)
    h64, s64 = ctc_fast.decode_beam_batch(torch.from_numpy(rows.astype(np.float64)).cuda(), lengths, beam=32, lm=lm)
    hl, sl = ctc_fast.decode_beam_batch(utts, beam=32, lm=lm)
    for b in range(3):
        assert list(h32[b]) == list(h64[b]) == list(hl[b])
    np.testing.assert_array_equal(s32, s64)
    np.testing.assert_array_equal(s32, sl)


def test_neg_inf_input_no_nan():
    import ctc_fast
    rs = np.random.RandomState(9)
    A, T = 8, 40
    lp = peaked(rs, A, T)
    mask = rs.rand(A, T) < 0.3
    mask[np.argmax(lp, axis=0), np.arange(T)] = False
    lp[mask] = -np.inf
    dead = lp.copy()
    dead[:, 17] = -np.inf                           # a frame where nothing is possible
    hyps, scores = ctc_fast.decode_beam_batch([lp, dead], beam=16, alpha=0.0, beta=1.0, nbest=4)
    assert not np.isnan(scores).any()
    top = beam_model.decode(lp, 16, 0.0, 1.0, None, nbest=2)
    assert_same(hyps[0][0], scores[0, 0], top[0][0], top[0][1], top[0][1] - top[1][1])
    assert np.all(scores[1] == -np.inf)


def test_t0_and_t1():
    import ctc_fast
    rs = np.random.RandomState(2)
    A = 35
    d = beam_decoder("5g")
    assert d.decode(np.asfortranarray(np.zeros((A, 0))), 40, 1.0, 0.0) == ("", 0.0)
    lp = peaked(rs, A, 1)
    lm = ctc_fast.DecodeLM(d.lm, d.int_char_map, A)
    hyps, scores = ctc_fast.decode_beam_batch([np.zeros((A, 0)), lp], beam=40, alpha=1.5, beta=0.5, lm=lm, nbest=2)
    assert len(hyps[0][0]) == 0 and scores[0, 0] == 0.0 and scores[0, 1] == -np.inf
    top = beam_model.decode(lp, 40, 1.5, 0.5, beam_model.arpa_rows(d.lm, lm.sym_words), nbest=2)
    assert_same(hyps[1][0], scores[1, 0], top[0][0], top[0][1], top[0][1] - top[1][1])


def test_limits_rejected():
    import ctc_fast
    lp = peaked(np.random.RandomState(0), 8, 10)
    for kw in (dict(beam=257), dict(beam=0), dict(nbest=5, beam=4)):
        with pytest.raises(ValueError):
            ctc_fast.decode_beam_batch([lp], **kw)
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch([np.zeros((257, 3))])
    d = beam_decoder("2g")
    with pytest.raises(ValueError):
        d.decode(np.asfortranarray(lp), 300, 1.0, 0.0)


def test_argmax_decoder():
    from new_decoder import decoder
    rs = np.random.RandomState(4)
    A, T = 10, 60
    lp = np.asfortranarray(peaked(rs, A, T))
    lp[:, 5] = lp[2, 5]                              # a tie: the first maximum wins
    a = decoder.ArgmaxDecoder()
    a.load_chars(CHARS)
    hyp, score = a.decode(lp)
    best = np.argmax(lp, axis=0)
    want, prev = [], -1
    for t in range(T):
        if best[t] != prev:
            prev = best[t]
            if prev > 0:
                want.append(a.int_char_map[int(prev)])
    assert hyp == "".join(want)
    assert score == pytest.approx(lp[best, np.arange(T)].sum(), rel=1e-12)


def test_run_decode_end_to_end(tmp_path):
    import dataLoader as dl
    import runDecode
    import writeLikelihoods as wl
    from nnets import brnnet
    rs = np.random.RandomState(0)
    raw = img = 12
    A = 6
    data = tmp_path / "data"
    data.mkdir()
    utts = [("u%d" % i, int(rs.randint(12, 30)), list(rs.randint(1, A, size=3))) for i in range(5)]
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
    out = tmp_path / "hyps.txt"
    cer = runDecode.main(["--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", str(chars),
                          "--alis", str(data / "alis1.txt"), "--lm", lm_path("2g"), "--out", str(out),
                          "--beam", "8", "--alpha", "0.5", "--batch", "2"])
    lines = out.read_text().splitlines()
    assert len(lines) == 5 and np.isfinite(cer) and cer >= 0
    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    from new_decoder import decoder
    d = decoder.BeamLMDecoder()
    d.load_chars(str(chars))
    d.load_lm(lm_path("2g"))
    for l in lines:
        parts = l.split(" ", 2)
        hyp, score = d.decode(np.asfortranarray(pk[parts[0]], dtype=np.float64), 8, 0.5, 0.0)
        assert float(parts[1]) == pytest.approx(score, abs=1e-6)
        assert (parts[2] if len(parts) > 2 else "") == hyp
