"""GPU checks of the recurrent character LM and of the prefix beam search that uses it (csrc/rnnlm.hip,
csrc/rnnlm_dev.h, ctc_rnnbeam_kernel in csrc/ctc_beam.hip).

The yardsticks are tests/rnn_lm_model.py (the float64 restatement of the model) and the unmodified
tests/beam_model.py / tests/beam_trace.py (the restatement of the search and the rules of
comparison).  Tolerance of rows and states, as in §4.7: for the same prefixes d32 = max |float32
evaluation accumulating in ascending k - float64| is computed in NumPy; the device may deviate from
float64 by at most 2 * d32 (partial sums in another order, the device's exp / log; a fused
multiply-add rounds less than NumPy's multiply then add).  Every model's Wh has a spectral norm below
1 (asserted), so that the float32 error of a state does not grow with the length of the prefix.  Every
precondition of a search comparison is asserted on the model before the GPU result is looked at;
seeds were chosen on the CPU with float64 rows standing in."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import beam_model
from tests import beam_trace as bt
from tests.beam_harness import PATTERN, int_char_map, raw_decode, same_results
from tests import rnn_lm_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "lm_char_rnn.npz")
CHARS = os.path.join(GOLDEN, "chars.txt")
NEG = float("-inf")


# name -> (seed, V, H); "fix" is tests/golden/lm_char_rnn.npz (V 37, H 64).  h40 is padded to 64, h1024
# takes four unit tiles per wave and pass, h2048 is the widest model the handle accepts.
MODELS = {"h40": (41, 38, 40), "h1024": (42, 40, 1024), "h2048": (43, 200, 2048)}
_HOST, _DEV, _D32 = {}, {}, {}


def host_lm(name):
    import nn_lm
    if name not in _HOST:
        lm = nn_lm.RNNCharLM.load(FIXTURE) if name == "fix" else M.random_lm(*MODELS[name])
        assert M.spectral_norm(lm.Wh) < 1, name
        _HOST[name] = lm
    return _HOST[name]


def sym_words(name, A):
    """the fixture maps chars.txt; a drawn model maps symbol c to id 3 + (c - 1) mod (V - 3)"""
    lm = host_lm(name)
    if name == "fix":
        return lm.symbol_words(int_char_map(), A)
    sw = np.zeros(A, dtype=np.int32)
    sw[1:] = 3 + (np.arange(1, A) - 1) % (lm.V - 3)
    return sw


def dev_lm(name, A):
    import ctc_fast
    if (name, A) not in _DEV:
        _DEV[(name, A)] = ctc_fast.DecodeRNNLM(host_lm(name), sym_words(name, A), A)
    return _DEV[(name, A)]


def device_rows_provider(dlm):
    """lm_row for beam_model.decode that returns exactly the float32 rows the kernel sees: DecodeRNNLM.rows,
    which keeps the states of the prefixes it has evaluated in ``cache``"""
    cache = {}

    def row(P):
        return dlm.rows([P], cache=cache)[0]
    return row


def chain_prefixes(A, n_seq, length, seed=100):
    """every prefix (length 0 .. ``length``) of ``n_seq`` random symbol sequences"""
    rs = np.random.RandomState(seed)
    seqs = [tuple(int(s) for s in rs.randint(1, A, size=length)) for _ in range(n_seq)]
    return [s[:n] for n in range(length + 1) for s in seqs]


ROW_SETS = {"fix": (8, 40), "h40": (8, 40), "h1024": (6, 40), "h2048": (3, 12)}


def yardstick(name):
    """(prefixes, float64 states, float64 rows, d32 of the states, d32 of the rows) of a model, once"""
    if name not in _D32:
        lm = host_lm(name)
        A = min(lm.V - 2, 35)
        sw = sym_words(name, A)
        prefixes = chain_prefixes(A, *ROW_SETS[name])
        ids = [[sw[s] for s in P] for P in prefixes]
        s64, r64 = M.forward64_many(lm, ids)
        s32, r32 = M.forward32(lm, ids)
        _D32[name] = (prefixes, s64, r64, np.abs(s32 - s64).max(), np.abs(r32 - r64).max())
    return _D32[name]


# ---- 1. rows and states against float64 ------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "h40", "h1024", "h2048"])
def test_rows_and_states_against_float64(name):
    """max |device - float64| <= 2 * d32 for the states and for the rows (DESIGN.md §4.10 lists d32 of
    the four models); the test prints the figures before it asserts."""
    lm = host_lm(name)
    A = min(lm.V - 2, 35)
    dlm = dev_lm(name, A)
    prefixes, s64, r64, d32_s, d32_r = yardstick(name)
    assert {len(P) for P in prefixes} == set(range(ROW_SETS[name][1] + 1))
    states = dlm.states(prefixes)
    rows = dlm.lm_rows(prefixes)
    assert states.dtype == np.float32 and states.shape == (len(prefixes), lm.H)
    assert rows.dtype == np.float32 and rows.shape == (len(prefixes), lm.V)
    dev_s = np.abs(states.astype(np.float64) - s64).max()
    dev_r = np.abs(rows.astype(np.float64) - r64).max()
    print("rnn %s: V %d H %d, %d prefixes of length 0..%d, rows span %.2f .. %.2g: states max |device - float64| "
          "= %.3g, d32 = %.3g (ratio %.2f); rows %.3g, d32 = %.3g (ratio %.2f)"
          % (name, lm.V, lm.H, len(prefixes), ROW_SETS[name][1], r64.min(), r64.max(), dev_s, d32_s, dev_s / d32_s,
             dev_r, d32_r, dev_r / d32_r))
    assert np.isfinite(rows).all() and np.isfinite(states).all() and (states >= 0).all()
    assert dev_s <= 2 * d32_s, (name, dev_s, d32_s)
    assert dev_r <= 2 * d32_r, (name, dev_r, d32_r)
    # the [n, A] view of the search: column 0 is 0, column c the row value of the symbol's LM id
    r = dlm.rows(prefixes[:20])
    assert r.shape == (20, A) and r.dtype == np.float32 and not r[:, 0].any()
    np.testing.assert_array_equal(r[:, 1:], rows[:20][:, dlm.sym_words[1:]])


# ---- 2. purity -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "h40", "h1024"])
def test_a_state_and_a_row_are_functions_of_the_prefix_alone(name):
    import torch
    lm = host_lm(name)
    A = min(lm.V - 2, 35)
    dlm = dev_lm(name, A)
    rs = np.random.RandomState(7)
    prefixes = [tuple(int(s) for s in rs.randint(1, A, size=rs.randint(0, 41))) for _ in range(300)]
    prefixes[0], prefixes[31], prefixes[32] = (), prefixes[31][:1] or (3,), ()
    assert max(len(P) for P in prefixes) == 40
    s300, r300 = dlm.states(prefixes), dlm.rows(prefixes)
    for i in (0, 31, 32, 150, 299):
        np.testing.assert_array_equal(dlm.rows(prefixes[i:i + 1])[0], r300[i])
        np.testing.assert_array_equal(dlm.states(prefixes[i:i + 1])[0], s300[i])
    pick = [299, 5, 64, 5, 33, 0, 150]
    np.testing.assert_array_equal(dlm.rows([prefixes[i] for i in pick]), r300[pick])
    np.testing.assert_array_equal(dlm.states([prefixes[i] for i in pick]), s300[pick])
    perm = rs.permutation(300)
    np.testing.assert_array_equal(dlm.rows([prefixes[i] for i in perm]), r300[perm])
    # one step of many pairs against the same pairs alone and elsewhere: more tiles than the step kernel
    # has workgroups (the grid-stride passes), NULL against an explicit zero state
    n = 2500
    ids = torch.from_numpy(rs.randint(0, lm.V, size=n).astype(np.int32)).cuda()
    base = torch.from_numpy(s300).cuda()
    sin = torch.zeros((n, dlm.Hp), dtype=torch.float32, device="cuda")
    sin[:, :lm.H] = base[torch.from_numpy(rs.randint(0, 300, size=n)).cuda()]
    so, ro = dlm.step(ids, sin)
    sub = torch.arange(0, n, 37, device="cuda")
    so2, ro2 = dlm.step(ids[sub].contiguous(), sin[sub].contiguous())
    assert torch.equal(so[sub], so2) and torch.equal(ro[sub], ro2)
    so3, none = dlm.step(ids[sub].contiguous(), sin[sub].contiguous(), rows=False)
    assert none is None and torch.equal(so3, so2)
    z0, zr0 = dlm.step(ids, None)
    z1, zr1 = dlm.step(ids, torch.zeros_like(sin))
    assert torch.equal(z0, z1) and torch.equal(zr0, zr1)
    bos = torch.tensor([lm.bos], dtype=torch.int32).cuda()
    np.testing.assert_array_equal(dlm.step(bos, None)[0].cpu().numpy()[0, :lm.H], s300[0])


# ---- 3. the rows the search used -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "h40", "h1024"])
def test_in_search_rows_equal_standalone_rows(name):
    """log10 P(c | prefix) read off the final beam of forced prefixes of length 1, 9 and 40 equals
    DecodeRNNLM.rows of the same prefixes to the read-off error"""
    import ctc_fast
    A, beam, alpha = 35, 40, 0.7
    dlm = dev_lm(name, A)
    rs = np.random.RandomState(31)
    prefixes = [tuple(int(s) for s in rs.randint(1, A, size=n)) for n in (0, 1, 1, 9, 9, 40, 40)]
    prefixes.append((5,) * 9)
    assert {len(P) for P in prefixes} >= {1, 9, 40}
    utts = [bt.forced_prefix_frames(rs, A, P) for P in prefixes]
    hyps, scores = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=alpha, beta=0.0, lm=dlm, nbest=beam)
    want = dlm.rows(prefixes)
    worst, pairs = 0.0, 0
    for b, (P, lp) in enumerate(zip(prefixes, utts)):
        row = bt.recover_lm_row(P, lp, hyps[b], scores[b], alpha)
        for c, (got, kmag) in row.items():
            bound = 1e-12 * kmag / alpha
            assert abs(got - float(want[b, c])) <= bound, (name, P, c, got, float(want[b, c]), bound)
            worst = max(worst, abs(got - float(want[b, c])) / bound)
            pairs += 1
    print("in-search rows %s: %d (prefix, symbol) pairs, worst error / bound %.3g" % (name, pairs, worst))
    assert pairs >= 34 * len(prefixes)


# ---- 4. the whole beam at every frame -------------------------------------------------------------------

def carried_input(rs, A, T, start, run, sharp=6.0):
    """bt.peaked with frames start .. start + run - 1 made blank-dominant: the best prefixes are carried
    through the run and extended after it"""
    lp = bt.peaked(rs, A, T)
    x = 1.5 * rs.randn(A, run)
    x[0] += sharp + 2.0
    lp[:, start:start + run] = bt.logsoftmax(x)
    return lp


def trace_facts(trace):
    """what a trace shows of the paths of step 4: the most new entries of one frame, the longest time a
    prefix had been carried when an extension of it entered the beam as a new entry, and how many
    entries re-entered the beam after having left it"""
    prev, age, seen = {()}, {(): 0}, {()}
    max_new = carried = reentered = 0
    for fr in trace:
        cur = [P for P, _ in fr["beam"]]
        new = [P for P, k in zip(cur, fr["kinds"]) if k == beam_model.EXT_CELL]
        assert all(P not in prev for P in new) and all(P in prev for P in cur if P not in new)
        max_new = max(max_new, len(new))
        for P in new:
            assert P[:-1] in prev
            carried = max(carried, age[P[:-1]])
            reentered += P in seen
        age = {P: (age[P] + 1 if P in prev else 0) for P in cur}
        prev = set(cur)
        seen |= prev
    return dict(new=max_new, carried=carried, reentered=reentered)


# (A, T, beam, model, alpha, beta, seed, float32 input, blank run or None, facts demanded of the trace)
# generator: bt.peaked / carried_input, RandomState(5000 + seed).  Seeds chosen on the model with float64
# rows for a defined cut and the facts; check_model and the facts are asserted on every run with the
# device's rows.
TRACE_INPUTS = [
    (35, 100, 64, "fix", 0.8, 0.5, 1, False, None, dict(new=33)),
    (8, 150, 16, "h40", 0.5, 1.5, 0, True, None, dict(reentered=1)),
    (20, 60, 200, "fix", 0.7, 0.3, 1, True, None, dict(new=33)),
    (30, 90, 40, "fix", 1.0, 0.3, 0, False, (30, 25), dict(carried=20)),
    (12, 80, 24, "h40", 1.3, 0.0, 0, True, (41, 24), dict(carried=20, reentered=1)),
    (33, 70, 48, "h1024", 1.5, 0.0, 1, False, (20, 21), dict(new=33, carried=20)),
]


def trace_input(A, T, seed, f32, run):
    rs = np.random.RandomState(5000 + seed)
    lp = bt.peaked(rs, A, T) if run is None else carried_input(rs, A, T, *run)
    return lp.astype(np.float32) if f32 else lp


@pytest.mark.parametrize("A,T,beam,name,alpha,beta,seed,f32,run,facts", TRACE_INPUTS)
def test_whole_beam_every_frame(A, T, beam, name, alpha, beta, seed, f32, run, facts):
    import ctc_fast
    lp = trace_input(A, T, seed, f32, run)
    dlm = dev_lm(name, A)
    trace = bt.model_trace(lp.astype(np.float64), beam, alpha, beta, device_rows_provider(dlm))
    st = bt.check_model(trace, beam)
    assert any(fr["cut"] is not None for fr in trace)
    got = trace_facts(trace)
    for k, v in facts.items():
        assert got[k] >= v, (k, got, facts)
    hyps, scores = ctc_fast.decode_beam_batch(bt.truncations(lp), beam=beam, alpha=alpha, beta=beta, lm=dlm,
                                              nbest=beam)
    worst = bt.compare(trace, hyps, scores, beam, what=(A, T, beam, name, seed))
    print("whole beam A=%d T=%d beam=%d lm=%s seed=%d %s: %d neighbour pairs, %d non-separated, most new entries "
          "of a frame %d, longest carry before an extension %d, re-entries %d, max |got-model|/|model| = %.3g"
          % (A, T, beam, name, seed, "f32" if f32 else "f64", st["pairs"], st["near"], got["new"], got["carried"],
             got["reentered"], worst))


# ---- 5. end to end against the float64 restatement --------------------------------------------------------

# seed of bt.peaked (RandomState(6000 + seed)) per case, chosen on the model with float64 rows so that the
# top-2 margin is at least ten times the tolerance; asserted on every run
E2E_SEEDS = list(range(24))


def e2e_cases():
    """(label, seed, beam, alpha, beta): the fixture LM, A = 35, T = 40"""
    cases = []
    for beam in (1, 16, 40, 150):
        for alpha in (0.0, 0.5, 1.3):
            for beta in (0.0, 1.5):
                cases.append(("b%d a%g b%g" % (beam, alpha, beta), E2E_SEEDS[len(cases)], beam, alpha, beta))
    return cases


def e2e_model(case, rows, d32):
    """(lp, best prefix, its key, tolerance, margin to the runner-up) of a case on the model"""
    label, seed, beam, alpha, beta = case
    lp = bt.peaked(np.random.RandomState(6000 + seed), 35, 40)
    trace = []
    top = beam_model.decode(lp, beam, alpha, beta, rows, nbest=2, trace=trace)
    P, k = top[0]
    t = bt.tol(k) + alpha * (len(P) + 1) * 2 * d32
    # the runner-up: the second entry of the beam, or (beam 1) the best candidate that was cut
    second = top[1][1] if len(top) > 1 else (trace[-1]["cut"] if trace and trace[-1]["cut"] is not None else NEG)
    return lp, P, k, t, k - second


def test_end_to_end_against_float64_rows():
    import ctc_fast
    A = 35
    lm = host_lm("fix")
    dlm = dev_lm("fix", A)
    d32 = yardstick("fix")[4]
    rows = M.rows64(lm, dlm.sym_words)
    cases = e2e_cases()
    assert len(cases) == 24
    worst = 0.0
    for case in cases:
        lp, P, k, t, margin = e2e_model(case, rows, d32)
        assert np.isfinite(k) and margin >= 10 * t, (case, k, t, margin)
        hyps, scores = ctc_fast.decode_beam_batch([lp], beam=case[2], alpha=case[3], beta=case[4], lm=dlm)
        assert abs(scores[0] - k) <= t, (case, scores[0], k, t)
        assert tuple(int(s) for s in hyps[0]) == P, (case, hyps[0], P, margin)
        worst = max(worst, abs(scores[0] - k) / t)
    print("end to end: %d cases, every hypothesis compared; worst |score - model| / tolerance %.3g; d32 = %.3g"
          % (len(cases), worst, d32))


# ---- 6. the C ABI below decode_beam_batch ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "h1024"])
def test_batch_composition_and_order(name):
    """an utterance decodes to the same bits alone, in a batch, and in the reversed batch"""
    import ctc_fast
    rs = np.random.RandomState(81)
    A, beam, nbest = 30, 24, 3
    dlm = dev_lm(name, A)
    utts = [bt.peaked(rs, A, T).astype(np.float32 if i % 2 else np.float64) for i, T in
            enumerate((40, 0, 7, 61, 1, 33, 18, 50, 25, 12))]
    kw = dict(beam=beam, alpha=0.9, beta=0.4, lm=dlm, nbest=nbest)
    h, s = ctc_fast.decode_beam_batch(utts, **kw)
    hr, sr = ctc_fast.decode_beam_batch(utts[::-1], **kw)
    same_results(h, s, hr[::-1], sr[::-1], nbest)
    for b in (0, 3, 7):
        h1, s1 = ctc_fast.decode_beam_batch([utts[b].astype(np.float64)], **kw)
        same_results(h1, s1, [h[b]], s[b], nbest)
    assert max(len(x[0]) for x in h) > 5 and np.isfinite(s[0]).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_ld_and_frame_offsets(dt):
    """ld > A with NaN in the padding columns, utterances in shuffled order with NaN-filled gaps"""
    import ctc_fast
    rs = np.random.RandomState(77)
    A, ld, beam, nbest = 35, 48, 24, 3
    dlm = dev_lm("fix", A)
    utts = [bt.peaked(rs, A, T).astype(dt) for T in (60, 1, 33, 0, 90, 17)]
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
    hyps, scores, lens, _, _ = raw_decode("rnnbeam", host, ld, A, T_b, frame_off, beam, nbest, dlm, 0.8, 0.5)
    ph, ps = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=nbest)
    assert not np.isnan(scores).any()
    same_results(hyps, scores, ph, ps, nbest)
    assert max(len(h[0]) for h in hyps) > 5


@pytest.mark.parametrize("name,nbest", [("fix", 1), ("fix", 16), ("h1024", 4)])
def test_exact_workspace_and_guarded_outputs(name, nbest):
    """nothing outside the workspace of exactly the advertised size, ids, lengths and scores is written:
    T = 0, T = 1 and long utterances mixed; the size is the formula of include/sctc.h"""
    import ctc_fast
    rs = np.random.RandomState(78)
    A, beam = 20, 16
    dlm = dev_lm(name, A)
    utts = [bt.peaked(rs, A, T) for T in (0, 150, 1, 0, 37, 1, 220)]
    T_b = [u.shape[1] for u in utts]
    host = np.ascontiguousarray(np.concatenate([u.T for u in utts], axis=0))
    frame_off = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    hyps, scores, lens, outside, nbytes = raw_decode("rnnbeam", host, A, A, T_b, frame_off, beam, nbest, dlm, 0.8,
                                                     beta=0.5, guard=4096)
    assert outside.size >= 5 * 4096 and np.all(outside == PATTERN)
    lm = host_lm(name)
    per_utt = 32 * beam * A + 8 * beam * dlm.Hp + 256 * dlm.Hp + 128 * ((lm.V + 31) // 32 * 32) + 512
    assert len(utts) * per_utt <= nbytes <= len(utts) * (per_utt + 8 * 256) + 4 * beam * sum(T_b) + 8 * 256 + 4096
    ph, ps = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=nbest)
    same_results(hyps, scores, ph, ps, nbest)
    assert scores[0, 0] == 0.0 and lens[0, 0] == 0 and (nbest == 1 or scores[0, 1] == NEG)


def test_beam_256_alphabet_256_hidden_2048():
    """the limits of the ABI on one utterance of 20 frames: 65 536 cells, the widest model, the best
    ranks against the model"""
    import ctc_fast
    A, T, beam, alpha, beta = 256, 20, 256, 0.6, 0.3
    dlm = dev_lm("h2048", A)
    lp = bt.peaked(np.random.RandomState(5), A, T)
    top = beam_model.decode(lp, beam, alpha, beta, device_rows_provider(dlm), nbest=3)
    hyps, scores = ctc_fast.decode_beam_batch([lp], beam=beam, alpha=alpha, beta=beta, lm=dlm, nbest=beam)
    assert np.isfinite(scores).all()
    for n in range(3):
        assert abs(scores[0, n] - top[n][1]) <= bt.tol(top[n][1]), (n, scores[0, n], top[n][1])
    if top[0][1] - top[1][1] > 2 * bt.tol(top[0][1]):
        assert tuple(int(s) for s in hyps[0][0]) == top[0][0]


def test_alpha_zero_with_an_lm_is_the_search_without():
    import ctc_fast
    rs = np.random.RandomState(9)
    A = 35
    dlm = dev_lm("fix", A)
    utts = [bt.peaked(rs, A, 50), bt.peaked(rs, A, 30).astype(np.float32)]
    utts[0][rs.rand(A, 50) < 0.2] = NEG
    h, s = ctc_fast.decode_beam_batch(utts, beam=16, alpha=0.0, beta=1.0, lm=dlm, nbest=4)
    h0, s0 = ctc_fast.decode_beam_batch(utts, beam=16, alpha=0.0, beta=1.0, lm=None, nbest=4)
    assert not np.isnan(s).any() and np.isfinite(s[:, 0]).all()
    same_results(h, s, h0, s0, 4)


def test_limits_rejected_and_handle_reports_its_bytes():
    import ctc_fast
    import _sctc
    dlm = dev_lm("fix", 35)
    assert dlm.device_bytes >= 4 * (64 * 37 + 64 * 64 + 64 + 64 * 64 + 64) + 64 * 256 * 64
    lp = bt.peaked(np.random.RandomState(0), 35, 10)
    for kw in (dict(beam=257), dict(beam=0), dict(nbest=5, beam=4)):
        with pytest.raises(ValueError):
            ctc_fast.decode_beam_batch([lp], lm=dlm, **kw)
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch([np.zeros((36, 3))], lm=dlm)          # more symbols than the map has
    with pytest.raises(ValueError):
        ctc_fast.DecodeRNNLM(host_lm("fix"), np.full(35, 37, dtype=np.int32))   # an id outside the vocabulary
    with pytest.raises(ValueError):
        dlm.rows([(1, 35)])                                              # a symbol the map does not have
    import torch
    ids4 = torch.zeros(4, dtype=torch.int32, device="cuda")
    for bad_state in (torch.zeros((4, dlm.Hp - 1), device="cuda"), torch.zeros((3, dlm.Hp), device="cuda"),
                      torch.zeros((4, dlm.Hp), dtype=torch.float64, device="cuda"), torch.zeros((4, dlm.Hp)),
                      torch.zeros((4, 2 * dlm.Hp), device="cuda")[:, ::2]):
        with pytest.raises(ValueError):
            dlm.step(ids4, bad_state)                                    # before anything is launched
    with pytest.raises(ValueError):
        dlm.step(ids4.long(), None)
    L = _sctc.lib()
    T, off = np.array([5], dtype=np.int32), np.zeros(1, dtype=np.int64)
    bad = np.full(35, 40, dtype=np.int32)
    cfg = _sctc.RNNBeamConfig(1, 35, _sctc.F32, 4, 1, 0, 35, _sctc.i32(T), _sctc.i64(off), 1.0, 0.0, dlm.handle,
                              _sctc.i32(bad))
    assert L.sctc_ctc_rnnbeam_workspace_bytes(ctypes.byref(cfg)) == 0 and b"LM id" in L.sctc_last_error()
    good = np.ascontiguousarray(dlm.sym_words)
    cfg.sym_word = _sctc.i32(good)
    for field, value, word in (("A", 257, b"alphabet"), ("A", 1, b"alphabet"), ("beam", 257, b"beam width"),
                               ("nbest", 5, b"nbest"), ("ld", 34, b"ld"), ("dtype", 7, b"dtype")):
        keep = getattr(cfg, field)
        setattr(cfg, field, value)
        assert L.sctc_ctc_rnnbeam_workspace_bytes(ctypes.byref(cfg)) == 0 and word in L.sctc_last_error(), field
        assert L.sctc_ctc_rnnbeam_decode_batch(ctypes.byref(cfg), None, None, None, None, None, 0, None) == -1
        setattr(cfg, field, keep)
    n = L.sctc_ctc_rnnbeam_workspace_bytes(ctypes.byref(cfg))
    assert n > 0
    import torch
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rc = L.sctc_ctc_rnnbeam_decode_batch(ctypes.byref(cfg), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                         buf.data_ptr(), buf.data_ptr(), n - 1, None)
    assert rc < 0 and b"workspace" in L.sctc_last_error()
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert L.sctc_rnnlm_step(dlm.handle, ids.data_ptr(), None, -1, buf.data_ptr(), None, None) == -1
    assert L.sctc_rnnlm_step(dlm.handle, ids.data_ptr(), None, 4, None, None, None) == -1
    assert b"null device pointer" in L.sctc_last_error()
    assert L.sctc_rnnlm_step(dlm.handle, None, None, 0, None, None, None) == 0


def test_run_decode_with_the_fixture_on_the_golden_shard(tmp_path):
    """runDecode.py --lm lm_char_rnn.npz: the golden shard through a BRNN, writeLikelihoods, and the
    recurrent-LM search with --ref-scores; every line equals BeamLMDecoder.decode of that utterance"""
    import dataLoader as dl
    import runDecode
    import writeLikelihoods as wl
    from new_decoder import decoder
    from nnets import brnnet
    g = np.load(os.path.join(GOLDEN, "loader_ref.npz"))
    raw = int(g["rawsize"])
    A = 35
    shard = os.path.join(GOLDEN, "shard")
    net = brnnet.NNet(raw, A, 32, 3, 200, train=False, temporalLayer=2)
    np.random.seed(1)
    net.initParams()
    loader = dl.DataLoader(shard + "/", raw, raw)
    lik = tmp_path / "lik"
    lik.mkdir()
    wl.writeLogLikes(loader, net, 1, str(lik), writePickle=True)
    out, ref = tmp_path / "hyps.txt", tmp_path / "ref.txt"
    cer = runDecode.main(["--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", CHARS,
                          "--alis", os.path.join(shard, "alis1.txt"), "--lm", FIXTURE, "--out", str(out),
                          "--beam", "8", "--alpha", "0.5", "--batch", "3", "--ref-scores", str(ref)])
    lines = out.read_text().splitlines()
    assert len(lines) == 4 and np.isfinite(cer) and cer >= 0
    assert len(ref.read_text().splitlines()) == 4
    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    d = decoder.BeamLMDecoder()
    d.load_chars(CHARS)
    d.load_lm(FIXTURE)
    import nn_lm
    assert isinstance(d.lm, nn_lm.RNNCharLM)
    for l in lines:
        parts = l.split(" ", 2)
        hyp, score = d.decode(np.asfortranarray(pk[parts[0]], dtype=np.float64), 8, 0.5, 0.0)
        assert float(parts[1]) == pytest.approx(score, abs=1e-6)
        assert (parts[2] if len(parts) > 2 else "") == hyp


def test_score_sentences_with_the_recurrent_lm():
    """score_sentences = log P_ctc + alpha * sum of the rows' values + beta * U, the rows being the
    device's own"""
    import ctc_fast
    A, alpha, beta = 35, 0.7, 0.4
    dlm = dev_lm("fix", A)
    rs = np.random.RandomState(12)
    utts = [bt.peaked(rs, A, T) for T in (40, 25, 60)]
    seqs = [rs.randint(1, A, size=n).astype(np.int32) for n in (6, 0, 11)]
    got = ctc_fast.score_sentences(utts, seqs, lm=dlm, alpha=alpha, beta=beta)
    _, _, _, total, status = ctc_fast.align_batch(utts, seqs, total=True)
    assert (status == 0).all()
    lmv = ctc_fast.lm_sentence_scores(seqs, dlm)
    for b, s in enumerate(seqs):
        prefixes = [tuple(int(c) for c in s[:i]) for i in range(len(s))]
        rows = dlm.rows(prefixes) if prefixes else np.zeros((0, A), np.float32)
        want_lm = sum(float(rows[i, int(c)]) for i, c in enumerate(s))
        assert lmv[b] == want_lm
        assert got[b] == total[b] + alpha * want_lm + beta * len(s)
    assert lmv[1] == 0.0 and lmv[0] < 0
