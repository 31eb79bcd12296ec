"""GPU checks of the neural character LM and of the prefix beam search that uses it (csrc/nnlm.hip,
csrc/nnlm_dev.h, ctc_nnbeam_kernel in csrc/ctc_beam.hip).

The yardsticks are tests/nn_lm_model.py (the float64 restatement of the model) and the unmodified
tests/beam_model.py / tests/beam_trace.py (the restatement of the search and the rules of
comparison).  Row tolerance: for the same contexts d32 = max |float32 evaluation accumulating in
ascending k - float64| is computed in NumPy; the device may deviate from float64 by at most 2 * d32
(partial sums in another order, the device's exp / log; a fused multiply-add rounds less than
NumPy's multiply then add).  Every precondition of a search comparison is asserted on the model
before the GPU result is looked at; seeds were chosen on the CPU with float64 rows standing in."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import beam_model
from tests import beam_trace as bt
from tests.beam_harness import PATTERN, int_char_map, raw_decode, same_results
from tests import nn_lm_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "lm_char_nn.npz")
CHARS = os.path.join(GOLDEN, "chars.txt")
NEG = float("-inf")


# name -> (seed, V, K, hidden, scale); "fix" is tests/golden/lm_char_nn.npz (V 37, K 8, 2 x 64)
MODELS = {
    "k3": (11, 38, 3, (64,), 1.5),
    "k12": (12, 38, 12, (96, 64), 1.5),
    "k19": (13, 40, 19, (1024, 1024), 1.5),
    "big": (14, 200, 32, (2048, 2048, 2048), 1.5),
    "odd": (15, 50, 5, (40, 72), 1.5),
    "v256": (16, 256, 2, (64,), 1.5),
}
_HOST, _DEV = {}, {}


def host_lm(name):
    import nn_lm
    if name not in _HOST:
        if name == "fix":
            _HOST[name] = nn_lm.NNCharLM.load(FIXTURE)
        else:
            seed, V, K, hidden, scale = MODELS[name]
            _HOST[name] = M.random_lm(seed, V, K, hidden, scale=scale)
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
        _DEV[(name, A)] = ctc_fast.DecodeNNLM(host_lm(name), sym_words(name, A), A)
    return _DEV[(name, A)]


def device_rows_provider(dlm):
    """lm_row for beam_model.decode that returns exactly the float32 rows the kernel sees"""
    cache = {}

    def row(P):
        key = tuple(int(i) for i in dlm.contexts([P])[0])
        if key not in cache:
            cache[key] = dlm.rows([P])[0]
        return cache[key]
    return row


def draw_contexts(lm, rs, n):
    """n windows: half random ids, half the padded windows of random prefixes of every length"""
    out = [rs.randint(0, lm.V, size=lm.context) for _ in range(n // 2)]
    while len(out) < n:
        L = int(rs.randint(0, lm.context + 6))
        out.append(lm.context_ids(rs.randint(3, lm.V, size=L)))
    return np.asarray(out, dtype=np.int32)


# ---- 1. rows against float64 -------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("fix", 400), ("k19", 300), ("big", 200), ("odd", 300)])
def test_rows_against_float64(name, n):
    """max |device - float64| <= 2 * d32; the test prints both figures before it asserts."""
    lm = host_lm(name)
    A = min(lm.V - 2, 35)
    dlm = dev_lm(name, A)
    ctx = draw_contexts(lm, np.random.RandomState(100), n)
    want = M.rows64_of_contexts(lm, ctx)
    d32 = np.abs(M.forward32(lm, ctx) - want).max()
    got = dlm.lm_rows(ctx)
    assert got.dtype == np.float32 and got.shape == (n, lm.V)
    dev = np.abs(got.astype(np.float64) - want).max()
    print("rows %s: V %d K %d hidden %s, %d contexts, rows span %.2f .. %.2g: max |device - float64| = %.3g, "
          "d32 = %.3g (ratio %.2f)" % (name, lm.V, lm.context, [w.shape[0] for w in lm.weights[:-1]], n,
                                        want.min(), want.max(), dev, d32, dev / d32))
    assert np.isfinite(got).all()
    assert dev <= 2 * d32, (name, dev, d32)
    # the [n, A] view of the search: column 0 is 0, column c the row value of the symbol's LM id
    prefixes = [tuple(int(s) for s in np.random.RandomState(i).randint(1, A, size=i % (lm.context + 4)))
                for i in range(20)]
    r = dlm.rows(prefixes)
    assert r.shape == (20, A) and r.dtype == np.float32 and not r[:, 0].any()
    full = dlm.lm_rows(dlm.contexts(prefixes))
    np.testing.assert_array_equal(r[:, 1:], full[:, dlm.sym_words[1:]])


# ---- 2. purity -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "k19", "odd"])
def test_a_row_is_a_function_of_its_context_alone(name):
    lm = host_lm(name)
    dlm = dev_lm(name, min(lm.V - 2, 35))
    rs = np.random.RandomState(7)
    ctx = draw_contexts(lm, rs, 300)
    all300 = dlm.lm_rows(ctx)
    for i in (0, 31, 32, 150, 299):
        np.testing.assert_array_equal(dlm.lm_rows(ctx[i:i + 1])[0], all300[i])
    seven = ctx[[299, 5, 64, 5, 33, 0, 150]]
    got7 = dlm.lm_rows(seven)
    np.testing.assert_array_equal(got7, all300[[299, 5, 64, 5, 33, 0, 150]])
    perm = rs.permutation(300)
    np.testing.assert_array_equal(dlm.lm_rows(ctx[perm]), all300[perm])
    # more tiles than the rows kernel has workgroups: the grid-stride passes
    many = ctx[rs.randint(0, 300, size=5000)]
    np.testing.assert_array_equal(dlm.lm_rows(many)[::37], dlm.lm_rows(many[::37]))


# ---- 3. the rows the search used ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "k3", "k12"])
def test_in_search_rows_equal_standalone_rows(name):
    """log10 P(c | prefix) read off the final beam of forced prefixes equals DecodeNNLM.rows of the same
    prefixes to the read-off error: prefixes shorter than, as long as and longer than the context"""
    import ctc_fast
    A, beam, alpha = 35, 40, 0.7
    lm = host_lm(name)
    dlm = dev_lm(name, A)
    K = lm.context
    rs = np.random.RandomState(31)
    prefixes = [tuple(int(s) for s in rs.randint(1, A, size=n)) for n in range(K + 4) for _ in range(2)]
    prefixes.append((5,) * (K + 1))
    assert {len(P) for P in prefixes} >= {0, 1, K - 1, K, K + 1, K + 3}
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

# (A, T, beam, model, alpha, beta, seed, float32 input); generator bt.peaked, RandomState(3000 + seed).
# Seeds chosen on the model with float64 rows for a defined cut; check_model asserts it on every run with
# the device's rows.
TRACE_INPUTS = [
    (35, 200, 16, "fix", 0.8, 0.5, 0, False),
    (35, 100, 64, "k12", 0.8, 0.5, 4, True),
    (8, 300, 24, "k3", 0.5, 1.5, 0, False),
    (12, 60, 200, "k12", 0.7, 0.3, 1, True),
    (33, 60, 40, "fix", 1.5, 0.0, 3, True),
    (20, 80, 40, "k19", 1.3, 0.0, 3, False),
    (35, 120, 40, "k3", 1.0, 0.3, 4, True),
]


@pytest.mark.parametrize("A,T,beam,name,alpha,beta,seed,f32", TRACE_INPUTS)
def test_whole_beam_every_frame(A, T, beam, name, alpha, beta, seed, f32):
    import ctc_fast
    lp = bt.peaked(np.random.RandomState(3000 + seed), A, T)
    if f32:
        lp = lp.astype(np.float32)
    dlm = dev_lm(name, A)
    trace = bt.model_trace(lp.astype(np.float64), beam, alpha, beta, device_rows_provider(dlm))
    st = bt.check_model(trace, beam)
    assert any(fr["cut"] is not None for fr in trace)
    hyps, scores = ctc_fast.decode_beam_batch(bt.truncations(lp), beam=beam, alpha=alpha, beta=beta, lm=dlm,
                                              nbest=beam)
    worst = bt.compare(trace, hyps, scores, beam, what=(A, T, beam, name, seed))
    print("whole beam A=%d T=%d beam=%d lm=%s (K %d) seed=%d %s: %d neighbour pairs, %d non-separated, "
          "max |got-model|/|model| = %.3g" % (A, T, beam, name, host_lm(name).context, seed,
                                              "f32" if f32 else "f64", st["pairs"], st["near"], worst))


# ---- 5. end to end against the float64 restatement --------------------------------------------------------

def e2e_cases():
    """(label, A x T input, beam, alpha, beta): the fixture LM, A = 35; generator bt.peaked,
    RandomState(4000 + i)"""
    cases = []
    i = 0
    for beam in (1, 16, 40, 150):
        for alpha in (0.0, 0.5, 1.3):
            for beta in (0.0, 1.5):
                cases.append(("b%d a%g b%g" % (beam, alpha, beta), ("peaked", 4000 + i, 40), beam, alpha, beta))
                i += 1
    for j, (beam, alpha, beta) in enumerate([(16, 0.5, 1.5), (40, 1.3, 0.0), (150, 0.5, 0.0)]):
        cases.append(("-inf %d" % j, ("masked", 4100 + j, 40), beam, alpha, beta))
    cases.append(("dead frame", ("dead", 4200, 30), 16, 0.5, 1.5))
    cases.append(("T=0", ("peaked", 4300, 0), 40, 1.3, 1.5))
    cases.append(("T=1", ("peaked", 4301, 1), 40, 1.3, 1.5))
    cases.append(("T=1 beam 1", ("peaked", 4302, 1), 1, 0.5, 0.0))
    return cases


def e2e_input(spec, A=35):
    kind, seed, T = spec
    rs = np.random.RandomState(seed)
    if T == 0:
        return np.zeros((A, 0))
    lp = bt.peaked(rs, A, T)
    if kind == "masked":
        mask = rs.rand(A, T) < 0.3
        mask[np.argmax(lp, axis=0), np.arange(T)] = False
        lp[mask] = NEG
    if kind == "dead":
        lp[:, 17] = NEG
    return lp


def test_end_to_end_against_float64_rows():
    import ctc_fast
    A = 35
    lm = host_lm("fix")
    dlm = dev_lm("fix", A)
    ctx = draw_contexts(lm, np.random.RandomState(100), 400)
    d32 = np.abs(M.forward32(lm, ctx) - M.rows64_of_contexts(lm, ctx)).max()
    rows = M.rows64(lm, dlm.sym_words)
    cases = e2e_cases()
    assert len(cases) >= 30
    under, compared = [], 0
    for label, spec, beam, alpha, beta in cases:
        lp = e2e_input(spec)
        trace = []
        top = beam_model.decode(lp, beam, alpha, beta, rows, nbest=2, trace=trace)
        hyps, scores = ctc_fast.decode_beam_batch([lp], beam=beam, alpha=alpha, beta=beta, lm=dlm)
        assert not np.isnan(scores).any()
        P, k = top[0]
        if k == NEG:
            assert scores[0] == NEG, (label, scores[0])
            continue
        t = bt.tol(k) + alpha * (len(P) + 1) * 2 * d32
        assert abs(scores[0] - k) <= t, (label, scores[0], k, t)
        # the runner-up: the second entry of the beam, or (beam 1) the best candidate that was cut
        second = top[1][1] if len(top) > 1 else (trace[-1]["cut"] if trace and trace[-1]["cut"] is not None else NEG)
        margin = k - second
        if margin > 2 * t:
            assert tuple(int(s) for s in hyps[0]) == P, (label, hyps[0], P, margin)
            compared += 1
        else:
            under.append(label)
    print("end to end: %d cases, %d hypotheses compared, under the margin: %s; d32 = %.3g"
          % (len(cases), compared, under, d32))
    assert len(under) <= 0.1 * len(cases), under


# ---- 6. the C ABI below decode_beam_batch ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fix", "k19"])
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
    hyps, scores, lens, _, _ = raw_decode("nnbeam", host, ld, A, T_b, frame_off, beam, nbest, dlm, 0.8, 0.5)
    ph, ps = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=nbest)
    assert not np.isnan(scores).any()
    same_results(hyps, scores, ph, ps, nbest)
    assert max(len(h[0]) for h in hyps) > 5


@pytest.mark.parametrize("name,nbest", [("fix", 1), ("fix", 16), ("k19", 4)])
def test_exact_workspace_and_guarded_outputs(name, nbest):
    """nothing outside the workspace of exactly the advertised size, ids, lengths and scores is written:
    T = 0, T = 1 and long utterances mixed"""
    import ctc_fast
    rs = np.random.RandomState(78)
    A, beam = 20, 16
    dlm = dev_lm(name, A)
    utts = [bt.peaked(rs, A, T) for T in (0, 150, 1, 0, 37, 1, 220)]
    T_b = [u.shape[1] for u in utts]
    host = np.ascontiguousarray(np.concatenate([u.T for u in utts], axis=0))
    frame_off = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    hyps, scores, lens, outside, nbytes = raw_decode("nnbeam", host, A, A, T_b, frame_off, beam, nbest, dlm, 0.8,
                                                     beta=0.5, guard=4096)
    assert outside.size >= 5 * 4096 and np.all(outside == PATTERN)
    lm = host_lm(name)
    hmax = max((w.shape[0] + 31) // 32 * 32 for w in lm.weights[:-1])
    per_utt = 32 * beam * A + 64 * beam + 256 * hmax + 128 * ((lm.V + 31) // 32 * 32) + 128 * lm.context
    assert len(utts) * per_utt <= nbytes <= len(utts) * (per_utt + 8 * 256) + 4 * beam * sum(T_b) + 8 * 256 + 4096
    ph, ps = ctc_fast.decode_beam_batch(utts, beam=beam, alpha=0.8, beta=0.5, lm=dlm, nbest=nbest)
    same_results(hyps, scores, ph, ps, nbest)
    assert scores[0, 0] == 0.0 and lens[0, 0] == 0 and (nbest == 1 or scores[0, 1] == NEG)


def test_beam_256_alphabet_256():
    """the limits of the ABI: 65 536 cells, a vocabulary of 256, every rank against the model"""
    import ctc_fast
    A, T, beam, alpha, beta = 256, 4, 256, 0.6, 0.3
    dlm = dev_lm("v256", A)
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
    assert dlm.device_bytes >= 4 * (64 * 296 + 64 * 64 + 64 * 64) + 64 * 256 * 64
    lp = bt.peaked(np.random.RandomState(0), 35, 10)
    for kw in (dict(beam=257), dict(beam=0), dict(nbest=5, beam=4)):
        with pytest.raises(ValueError):
            ctc_fast.decode_beam_batch([lp], lm=dlm, **kw)
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch([np.zeros((36, 3))], lm=dlm)          # more symbols than the map has
    with pytest.raises(ValueError):
        ctc_fast.DecodeNNLM(host_lm("fix"), np.full(35, 37, dtype=np.int32))   # an id outside the vocabulary
    with pytest.raises(ValueError):
        dlm.lm_rows(np.full((2, 8), 37))
    L = _sctc.lib()
    T, off = np.array([5], dtype=np.int32), np.zeros(1, dtype=np.int64)
    bad = np.full(35, 40, dtype=np.int32)
    cfg = _sctc.NNBeamConfig(1, 35, _sctc.F32, 4, 1, 0, 35, _sctc.i32(T), _sctc.i64(off), 1.0, 0.0, dlm.handle,
                             _sctc.i32(bad))
    assert L.sctc_ctc_nnbeam_workspace_bytes(ctypes.byref(cfg)) == 0 and b"LM id" in L.sctc_last_error()
    good = np.ascontiguousarray(dlm.sym_words)
    cfg.sym_word = _sctc.i32(good)
    n = L.sctc_ctc_nnbeam_workspace_bytes(ctypes.byref(cfg))
    assert n > 0
    import torch
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rc = L.sctc_ctc_nnbeam_decode_batch(ctypes.byref(cfg), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                        buf.data_ptr(), buf.data_ptr(), n - 1, None)
    assert rc < 0 and b"workspace" in L.sctc_last_error()


def test_run_decode_with_the_fixture_on_the_golden_shard(tmp_path):
    """runDecode.py --lm lm_char_nn.npz: the golden shard through a BRNN, writeLikelihoods, and the
    neural-LM search; every line equals BeamLMDecoder.decode of that utterance"""
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
    out = tmp_path / "hyps.txt"
    cer = runDecode.main(["--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", CHARS,
                          "--alis", os.path.join(shard, "alis1.txt"), "--lm", FIXTURE, "--out", str(out),
                          "--beam", "8", "--alpha", "0.5", "--batch", "3"])
    lines = out.read_text().splitlines()
    assert len(lines) == 4 and np.isfinite(cer) and cer >= 0
    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    d = decoder.BeamLMDecoder()
    d.load_chars(CHARS)
    d.load_lm(FIXTURE)
    import nn_lm
    assert isinstance(d.lm, nn_lm.NNCharLM)
    for l in lines:
        parts = l.split(" ", 2)
        hyp, score = d.decode(np.asfortranarray(pk[parts[0]], dtype=np.float64), 8, 0.5, 0.0)
        assert float(parts[1]) == pytest.approx(score, abs=1e-6)
        assert (parts[2] if len(parts) > 2 else "") == hyp
