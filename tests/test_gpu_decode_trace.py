"""GPU checks of the prefix beam search decoder beyond its winner (csrc/ctc_beam.hip, DESIGN.md
§4.5): the whole beam after every frame against the Python restatement (every rank's key and
hypothesis, so every rank's back-pointer walk), the reference's own top entry after every frame
(tests/golden/decode_ref_trace.npz), the device LM rows against a textbook back-off, the tie
rule of the select, and the corners of the C ABI that ``decode_beam_batch`` never uses (ld > A,
arbitrary frame offsets, an exact workspace, guarded output buffers, a batch larger than the part).

tests/beam_trace.py has the rules of comparison.  Every precondition (cut gap, share of
non-separated neighbours, one-kind ties) is asserted on the model before the GPU is touched."""
import os

import numpy as np
import pytest

from tests import beam_model
from tests import beam_trace as bt
from tests.beam_harness import PATTERN, int_char_map, raw_decode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEG = float("-inf")


_LMS = {}


def lms(k, A):
    """(ArpaLM, DecodeLM, model rows) of a fixture LM for an alphabet of A symbols"""
    import arpa_lm
    import ctc_fast
    if k is None:
        return None, None, None
    if (k, A) not in _LMS:
        alm = arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_%s.arpa" % k))
        dlm = ctc_fast.DecodeLM(alm, int_char_map(), A)
        _LMS[(k, A)] = (alm, dlm, beam_model.arpa_rows(alm, dlm.sym_words))
    return _LMS[(k, A)]


def decode_truncations(lp, beam, alpha, beta, dlm):
    import ctc_fast
    return ctc_fast.decode_beam_batch(bt.truncations(lp), beam=beam, alpha=alpha, beta=beta, lm=dlm, nbest=beam)


# ---- the whole beam at every frame -----------------------------------------------------------

# (A, T, beam, lm, alpha, beta, seed, float32 input); generator bt.peaked, RandomState(1000 + seed).
# Seeds chosen on the model for a comfortable cut gap; check_model asserts it on every run.
TRACE_INPUTS = [
    (35, 200, 16, "5g", 0.8, 0.5, 1, False),
    (35, 200, 16, "5g", 0.8, 0.5, 5, True),
    (8, 300, 24, "2g", 0.5, 1.5, 2, False),
    (8, 300, 24, "2g", 0.5, 1.5, 4, True),
    (35, 100, 64, None, 0.0, 0.3, 4, False),
    (35, 100, 64, None, 0.0, 0.3, 0, True),
    (12, 60, 200, None, 0.0, 0.3, 1, False),      # beam > A * n in the first frames: nothing is cut
    (12, 60, 200, None, 0.0, 0.3, 5, True),
    (33, 60, 40, "2g", 1.5, 0.0, 0, False),
    (33, 60, 40, "2g", 1.5, 0.0, 4, True),
    (33, 80, 40, "5g", 1.3, 0.0, 4, False),
    (33, 80, 40, "5g", 1.3, 0.0, 2, True),
]


@pytest.mark.parametrize("A,T,beam,lm,alpha,beta,seed,f32", TRACE_INPUTS)
def test_whole_beam_every_frame(A, T, beam, lm, alpha, beta, seed, f32):
    """Largest |got - model| / |model| over all keys of all twelve inputs on an MI355X: see
    DESIGN.md §4.5 (the test prints it)."""
    lp = bt.peaked(np.random.RandomState(1000 + seed), A, T)
    if f32:
        lp = lp.astype(np.float32)
    _, dlm, rows = lms(lm, A)
    trace = bt.model_trace(lp.astype(np.float64), beam, alpha, beta, rows)
    st = bt.check_model(trace, beam)
    if beam > A:
        assert trace[0]["cut"] is None and len(trace[0]["beam"]) < beam      # early frames keep everything
    assert any(fr["cut"] is not None for fr in trace)
    hyps, scores = decode_truncations(lp, beam, alpha, beta, dlm)
    worst = bt.compare(trace, hyps, scores, beam, what=(A, T, beam, lm, seed))
    print("whole beam A=%d T=%d beam=%d lm=%s seed=%d %s: %d neighbour pairs, %d non-separated, "
          "max |got-model|/|model| = %.3g" % (A, T, beam, lm, seed, "f32" if f32 else "f64", st["pairs"],
                                              st["near"], worst))


def test_reference_truncations():
    """the reference's own top entry after every frame, alpha / beta that are no float32 numbers"""
    z = np.load(os.path.join(GOLDEN, "decode_ref_trace.npz"))
    import ctc_fast
    compared = 0
    for i in range(int(z["n"])):
        A, T, beam = (int(v) for v in z["cfg%d" % i][:3])
        alpha, beta = float(z["cfg%d" % i][3]), float(z["cfg%d" % i][4])
        lp = z["lp%d" % i]
        _, dlm, rows = lms(str(z["lm%d" % i]), A)
        trace = bt.model_trace(lp, beam, alpha, beta, rows)
        hyps, scores = ctc_fast.decode_beam_batch(bt.truncations(lp), beam=beam, alpha=alpha, beta=beta, lm=dlm)
        ends = np.cumsum(z["len%d" % i])
        for t in range(T):
            ref = float(z["score%d" % i][t])
            assert abs(scores[t] - ref) <= 1e-6 * abs(ref) + 1e-9, (i, t, scores[t], ref)
            keys = [k for _, k in trace[t]["beam"]]
            if len(keys) < 2 or keys[0] - keys[1] >= 1e-6:
                assert list(hyps[t]) == list(z["hyp%d" % i][ends[t] - z["len%d" % i][t]:ends[t]]), (i, t)
                compared += 1
    assert compared >= 200


# ---- LM rows ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", ["2g", "5g"])
def test_lm_rows_against_textbook_backoff(k):
    """log10 P(c | <s> P) of the device LM lookup, read off the final beam of forced prefixes, against
    a float64 back-off over ArpaLM.ngrams, term by term"""
    import ctc_fast
    A, beam, alpha = 35, 40, 0.7
    alm, dlm, _ = lms(k, A)
    sw = dlm.sym_words
    rs = np.random.RandomState(31)
    prefixes = bt.lm_row_prefixes(alm, sw, rs)
    utts = [bt.forced_prefix_frames(rs, A, P) for P in prefixes]
    assert float(np.float32(alpha)) != alpha
    assert {len(P) for P in prefixes} >= set(range(alm.order + 3))
    assert any(len(P) > 1 and P[-1] == P[-2] for P in prefixes)
    unk = [s for s in range(1, A) if sw[s] == alm.unk]
    assert 4 in unk and 34 in unk and all(any(s in P for P in prefixes) for s in (4, 34))
    assert ((alm.unk,) in alm.ngrams) and (("<unk>" in open(os.path.join(GOLDEN, "lm_char_%s.arpa" % k)).read())
                                           == (k == "5g"))
    hyps, scores = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=alpha, beta=0.0, lm=dlm, nbest=beam)
    rows = [bt.recover_lm_row(P, lp, hyps[b], scores[b], alpha) for b, (P, lp) in enumerate(zip(prefixes, utts))]
    st = bt.check_lm_rows(alm, sw, prefixes, rows, alpha, what=k)
    print("lm rows %s: %d (P, c) pairs, longest match at n = %s, %d early chain breaks, %d full chains, "
          "worst error / bound %.3g; %d single-term values, worst relative error %.3g"
          % (k, st["pairs"], sorted(st["match"]), st["early_break"], st["full_chain"], st["worst"], st["single"],
             st["worst_single"]))
    assert st["pairs"] >= 200 and st["match"] == set(range(1, alm.order + 1)) and st["full_chain"] >= 50
    assert st["single"] >= 50
    if alm.order > 2:
        assert st["early_break"] >= 50


# ---- ties --------------------------------------------------------------------------------------

TIE_INPUTS = [   # (name, A, T, beam, lm, alpha, beta, seed)
    ("sparse", 8, 40, 32, None, 0.0, 0.4, 0),
    ("sparse", 8, 40, 32, "2g", 0.7, 0.4, 2),
    ("dead", 8, 40, 32, None, 0.0, 0.4, 1),
    ("dead", 8, 40, 32, "2g", 0.7, 0.4, 2),
    ("dead256", 256, 5, 256, None, 0.0, 0.3, 2),
]


@pytest.mark.parametrize("name,A,T,beam,lm,alpha,beta,seed", TIE_INPUTS)
def test_neg_inf_ties_in_cell_order(name, A, T, beam, lm, alpha, beta, seed):
    """more -inf candidates than free places: the first in cell order are kept, in that order"""
    if name == "sparse":
        lp = bt.sparse_frames(np.random.RandomState(2000 + seed), A, T)
    elif name == "dead":
        lp = bt.dead_frame(np.random.RandomState(2100 + seed), A, T, 12)
    else:
        lp = bt.dead_frame(np.random.RandomState(2300 + seed), A, T, 2)
    _, dlm, rows = lms(lm, A)
    trace = bt.model_trace(lp, beam, alpha, beta, rows)
    # no finite pair may swap: the order of the -inf cells hangs on the ranks of their parents
    st = bt.check_model(trace, beam, near_cap=0.0)
    assert 2 * st["cut_in_inf_tie"] >= T, st
    if name == "dead256":
        assert len(trace[1]["beam"]) == 256 and trace[2]["cut"] == NEG       # 65 536 cells in the tie scan
    hyps, scores = decode_truncations(lp, beam, alpha, beta, dlm)
    bt.compare(trace, hyps, scores, beam, what=(name, seed))
    print("-inf ties %s seed %d: %d of %d frames cut inside a -inf tie, %d -inf neighbour pairs in order"
          % (name, seed, st["cut_in_inf_tie"], T, st["inf_ties"]))


@pytest.mark.parametrize("seed", [0, 2, 4, 7])
def test_twin_symbols_exact_ties(seed):
    """two pairs of symbols with identical columns: bit-equal finite keys, at neighbours and at the
    cut; the model's exact order and membership are demanded"""
    A, T, beam = 7, 40, 12
    lp = bt.twins(np.random.RandomState(2200 + seed), A, T, [(1, 2), (4, 6)])
    trace = bt.model_trace(lp, beam, 0.0, 0.3, None)
    st = bt.check_model(trace, beam, exact_ties=True)
    assert st["ties"] >= 300 and st["cut_in_tie"] >= 5 and st["near"] == 0, st
    hyps, scores = decode_truncations(lp, beam, 0.0, 0.3, None)
    bt.compare(trace, hyps, scores, beam, exact_ties=True, what=("twins", seed))
    print("twins seed %d: %d exact neighbour ties of %d pairs, %d frames cut inside an exact tie"
          % (seed, st["ties"], st["pairs"], st["cut_in_tie"]))


# ---- the C ABI below decode_beam_batch -------------------------------------------------------

@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ld_and_frame_offsets(dt):
    """ld > A with NaN in the padding columns, utterances in shuffled order with NaN-filled gaps"""
    import ctc_fast
    rs = np.random.RandomState(77)
    A, ld, beam, nbest = 35, 48, 24, 3
    _, dlm, _ = lms("5g", A)
    utts = [bt.peaked(rs, A, T).astype(dt) for T in (60, 1, 33, 0, 90, 17)]
    T_b = [u.shape[1] for u in utts]
    order = [4, 0, 5, 2, 3, 1]                       # where each utterance lies in the matrix
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
    hyps, scores, lens, _, _ = raw_decode("beam", host, ld, A, T_b, frame_off, beam, nbest, dlm, 0.8, 0.5)
    ph, ps = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=nbest)
    np.testing.assert_array_equal(scores, ps)
    assert not np.isnan(scores).any()
    for b in range(len(utts)):
        for n in range(nbest):
            np.testing.assert_array_equal(hyps[b][n], ph[b][n])
    assert max(len(h[0]) for h in hyps) > 5


@pytest.mark.parametrize("lm,nbest", [(None, 1), (None, 16), ("2g", 1), ("2g", 16)])
def test_exact_workspace_and_guarded_outputs(lm, nbest):
    """nothing outside the workspace of exactly the advertised size, ids, lengths and scores is
    written: T = 0, T = 1 and long utterances mixed"""
    import ctc_fast
    rs = np.random.RandomState(78)
    A, beam = 20, 16
    _, dlm, _ = lms(lm, A)
    utts = [bt.peaked(rs, A, T) for T in (0, 150, 1, 0, 37, 1, 220)]
    T_b = [u.shape[1] for u in utts]
    host = np.ascontiguousarray(np.concatenate([u.T for u in utts], axis=0))
    frame_off = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    hyps, scores, lens, outside, _ = raw_decode("beam", host, A, A, T_b, frame_off, beam, nbest, dlm, 0.8, 0.5,
                                                guard=4096)
    assert outside.size >= 5 * 4096 and np.all(outside == PATTERN)
    ph, ps = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=nbest)
    np.testing.assert_array_equal(scores, np.asarray(ps).reshape(len(utts), nbest))
    for b in range(len(utts)):
        got = hyps[b]
        want = ph[b] if nbest > 1 else [ph[b]]
        for n in range(nbest):
            np.testing.assert_array_equal(got[n], want[n])
    assert scores[0, 0] == 0.0 and lens[0, 0] == 0 and (nbest == 1 or scores[0, 1] == NEG)


def test_batch_of_1200_equals_one_by_one():
    """more workgroups than the part has compute units, several rounds of them"""
    import ctc_fast
    rs = np.random.RandomState(79)
    A, beam = 20, 8
    _, dlm, _ = lms("2g", A)
    utts = [bt.peaked(rs, A, int(rs.randint(0, 13))) for _ in range(1200)]
    hyps, scores = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=2)
    assert scores.shape == (1200, 2)
    for b in range(0, 1200):
        h1, s1 = ctc_fast.decode_beam_batch([utts[b]], beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=2)
        np.testing.assert_array_equal(s1[0], scores[b])
        for n in range(2):
            np.testing.assert_array_equal(h1[0][n], hyps[b][n])
