"""GPU checks of the CTC forced alignment and sentence scoring (csrc/ctc_align.hip).
Everything is checked against the NumPy model of the contract (tests/align_model.py): paths, spans and
status equal, the Viterbi score bit-equal, the total to rel 1e-11."""
import ctypes
import itertools
import os
import pickle

import numpy as np
import pytest

from tests import align_model as am
from tests import beam_model
from tests.test_dataloader import write_shard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOTAL_RTOL = 1e-11

# score_sentences against the search (test_score_sentences_against_the_search): the worst gap, measured on
# the CPU over the test's own inputs between tests/beam_model.py (float32 masses between frames) and the
# float64 model, see search_gap_on_the_host(); the test allows four times that
SEARCH_GAP_MEASURED = 8.7e-08
SEARCH_MARGIN = 4 * SEARCH_GAP_MEASURED


def log_softmax_cols(z):
    z = z - z.max(axis=0, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=0, keepdims=True))


def rand_y(rs, A, T, dtype=np.float64):
    return np.asfortranarray(log_softmax_cols(rs.randn(A, T) * 2.0).astype(dtype))


def rand_labels(rs, U, A, blank=0):
    syms = [c for c in range(A) if c != blank]
    l = np.array([syms[i] for i in rs.randint(0, len(syms), size=U)], dtype=np.int32)
    if U >= 4:
        l[U // 2] = l[U // 2 - 1]       # at least one repeat
    return l


def repeats(l):
    return int(np.sum(np.asarray(l[1:]) == np.asarray(l[:-1]))) if len(l) > 1 else 0


def assert_same(got, want, what=""):
    fl, sp, vit, tot, st = got
    wfl, wsp, wvit, wtot, wst = want
    assert np.array_equal(st, wst), (what, st, wst)
    assert vit.dtype == np.float64 and np.array_equal(vit, wvit), (what, vit, wvit)     # bit-equal
    for b in range(len(wfl)):
        assert fl[b].dtype == np.int32 and np.array_equal(fl[b], wfl[b]), (what, b, fl[b], wfl[b])
        assert sp[b].shape == wsp[b].shape and np.array_equal(sp[b], wsp[b]), (what, b, sp[b], wsp[b])
    if wtot is None:
        assert tot is None
    else:
        fin = np.isfinite(wtot)
        assert np.array_equal(tot[~fin], wtot[~fin]), (what, tot, wtot)
        assert np.all(np.abs(tot[fin] - wtot[fin]) <= TOTAL_RTOL * np.abs(wtot[fin])), (what, tot, wtot)


def check(ys, seqs, blank=0, what=""):
    """one batched call with and one without the total, against the model; returns the device result"""
    import ctc_fast
    with np.errstate(all="ignore"):
        want = am.align_batch(ys, seqs, blank, total=True)
    got = ctc_fast.align_batch(ys, seqs, blank=blank, total=True)
    assert_same(got, want, what)
    plain = ctc_fast.align_batch(ys, seqs, blank=blank)
    assert_same(plain, want[:3] + (None,) + want[4:], what)
    return got


def same_bits(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_enumeration_shapes_in_one_batch():
    rs = np.random.RandomState(11)
    rows = [list(r) for n in range(4) for r in itertools.product((1, 2), repeat=n)]
    ys, seqs = [], []
    for T in range(1, 6):
        y = rand_y(rs, 3, T)
        for l in rows:
            ys.append(y)
            seqs.append(l)
    got = check(ys, seqs, what="enumeration")
    n_bad = 0
    for b, (y, l) in enumerate(zip(ys, seqs)):
        v, t = am.enumerate_paths(y, l)
        n_bad += v == -np.inf
        assert got[4][b] == (1 if v == -np.inf else 0)
        assert got[2][b] == v
        assert got[3][b] == t or abs(got[3][b] - t) <= TOTAL_RTOL * abs(t)
    assert n_bad >= 20


@pytest.mark.parametrize("A", [2, 33])
@pytest.mark.parametrize("U", [0, 1, 31, 32, 63, 64, 127, 128, 255])
def test_lane_boundaries_of_the_wave_path(U, A):
    import ctc_fast
    assert ctc_fast.align_plan(U)["path"] == "wave"
    rs = np.random.RandomState(100 * U + A)
    l = rand_labels(rs, U, A)
    tight = U + repeats(l)              # the single path without blanks
    Ts = [tight, tight + 1, 2 * U + 5]
    got = check([rand_y(rs, A, T) for T in Ts], [l] * 3, what="U=%d A=%d" % (U, A))
    assert list(got[4]) == [0, 0, 0]
    assert np.sum(got[0][0] < 0) == repeats(l)      # the single path: a blank only between equal labels


@pytest.mark.parametrize("U", [256, 700])
def test_wide_path(U):
    import ctc_fast
    assert ctc_fast.align_plan(U)["path"] == "wide"
    rs = np.random.RandomState(U)
    l = rand_labels(rs, U, 33)
    check([rand_y(rs, 33, 1100), rand_y(rs, 33, U + repeats(l))], [l, l], what="wide U=%d" % U)


def test_wide_path_at_the_length_limit():
    """U = 4095: 8191 states on 1024 threads, the largest edge arrays and the smallest staging block (8 frames)"""
    import ctc_fast
    U = ctc_fast._sctc.ALIGN_MAX_U
    plan = ctc_fast.align_plan(U)
    assert (plan["path"], plan["nl"], plan["stage_frames"]) == ("wide", 1024, 8)
    rs = np.random.RandomState(4095)
    l = rand_labels(rs, U, 33)
    got = check([rand_y(rs, 33, U + repeats(l) + 3)], [l], what="U=4095")
    assert got[4][0] == 0
    with pytest.raises(ValueError, match="4095"):
        ctc_fast.align_batch([rand_y(rs, 33, 4)], [np.ones(U + 1, np.int32)])
    with pytest.raises(ValueError, match="4095"):
        ctc_fast.align_batch([rand_y(rs, 33, 4)], [np.ones(9000, np.int32)])


@pytest.mark.parametrize("U", [0, 1, 64, 255])
def test_both_paths_agree_bit_for_bit(U, monkeypatch):
    import ctc_fast
    rs = np.random.RandomState(7 + U)
    l = rand_labels(rs, U, 9)
    ys = [rand_y(rs, 9, T) for T in (U + repeats(l), 2 * U + 3, 3 * U + 2)]
    monkeypatch.setenv("SCTC_ALIGN_PATH", "wide")
    assert ctc_fast.align_plan(U, "wide")["spl"] == 8
    wide = check(ys, [l] * 3, what="forced wide U=%d" % U)
    monkeypatch.setenv("SCTC_ALIGN_PATH", "wave")
    wave = check(ys, [l] * 3, what="forced wave U=%d" % U)
    same_bits(wave, wide)
    monkeypatch.delenv("SCTC_ALIGN_PATH")
    same_bits(ctc_fast.align_batch(ys, [l] * 3, total=True), wave)


@pytest.mark.parametrize("U,path", [(10, None), (50, None), (100, None), (200, None), (300, None), (10, "wide")])
def test_back_pointer_storage_thresholds(U, path, monkeypatch):
    """T one below, at and one above the largest T whose back-pointers stay on chip, and -- beyond it -- one
    below, at and one above a whole number of the trace-back's staging blocks"""
    import ctc_fast
    if path:
        monkeypatch.setenv("SCTC_ALIGN_PATH", path)
    plan = ctc_fast.align_plan(U, path)
    lds, blk = plan["lds_frames"], plan["stage_frames"]
    assert lds % blk == 0 and blk % plan["fpw"] == 0
    rs = np.random.RandomState(U)
    l = rand_labels(rs, U, 5)
    far = (max(lds, U + repeats(l)) // blk + 1) * blk    # a whole number of blocks, beyond the chip and long enough to align
    Ts = [lds - 1, lds, lds + 1, far - 1, far, far + 1]
    ymax = rand_y(rs, 5, max(Ts))
    ys = [np.asfortranarray(ymax[:, :T]) for T in Ts]
    L = ctc_fast._sctc.lib()
    got = check(ys, [l] * len(Ts), what="storage U=%d %s" % (U, plan))
    assert np.all(got[4][3:] == 0) and (U > 200 or np.all(got[4] == 0))
    # the threshold is where the test believes it is: the first three utterances need no workspace
    n = ctypes.c_size_t(0)
    for T, want_ws in ((lds, False), (lds + 1, True)):
        Tb, Ub, z = np.array([T], np.int32), np.array([U], np.int32), np.zeros(1, np.int64)
        cfg = ctc_fast._sctc.AlignConfig(1, 5, 0, 0, 5, 0, ctc_fast._sctc.i32(Tb), ctc_fast._sctc.i64(z),
                                         ctc_fast._sctc.i32(Ub), ctc_fast._sctc.i64(z))
        assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
        assert (n.value > 0) == want_ws, (T, n.value)


def test_ties_follow_the_rule():
    rs = np.random.RandomState(3)
    ys, seqs = [], []
    for T, l in ((6, [1, 2]), (6, [1, 1]), (6, [1, 2, 1]), (3, [1, 2, 1]), (2, [1]), (9, [2, 2, 2]), (40, [1, 2, 3, 3, 1])):
        ys.append(np.full((4, T), -1.0))                            # all-equal lattices
        seqs.append(l)
    y = np.full((4, 2), -1.0)
    y[0, 1] = -1.5                                                  # S-2 strictly better at the end
    ys.append(y)
    seqs.append([1])
    for T, U in ((7, 3), (30, 9), (64, 20), (200, 70)):             # a 1/8 grid: sums are exact, ties are common
        ys.append(np.asfortranarray(-rs.randint(0, 4, size=(4, T)) / 8.0))
        seqs.append(rand_labels(rs, U, 4))
    got = check(ys, seqs, what="ties")
    fl = got[0]
    assert list(fl[0]) == [0, 1, -1, -1, -1, -1] and list(fl[1]) == [0, -1, 1, -1, -1, -1]
    assert list(fl[2]) == [0, 1, 2, -1, -1, -1] and list(fl[3]) == [0, 1, 2]
    assert list(fl[4]) == [0, -1] and list(fl[7]) == [0, 0]
    assert np.array_equal(got[2][:5], [-6.0, -6.0, -6.0, -3.0, -2.0])
    # the same on the wide kernel and with eight states a lane
    U = 150
    l = rand_labels(rs, U, 4)
    check([np.asfortranarray(-rs.randint(0, 4, size=(4, 2 * U + 9)) / 8.0), np.full((4, 2 * U + 40), -0.5)], [l, l], what="ties, 8 a lane")


def test_minus_inf():
    rs = np.random.RandomState(4)
    y = np.full((3, 5), -np.inf)
    for t, c in enumerate([0, 1, 1, 0, 2]):     # one finite symbol per frame: the path is forced
        y[c, t] = -0.5 * (t + 1)
    y2 = rand_y(rs, 3, 5)
    y2[:, 2] = -np.inf                          # a frame of all -inf
    y3 = rand_y(rs, 3, 6)
    y3[0, 3] = y3[1, 3] = -np.inf               # the lattice of [1] is cut in the middle
    y4 = rand_y(rs, 5, 90)
    y4[:, 40:50] = -np.inf
    l4 = rand_labels(rs, 30, 5)
    y4[l4[12], 40:50] = -1.0                    # ten frames that only label 12 survives
    with np.errstate(all="ignore"):
        holes = np.where(rs.rand(5, 90) < 0.3, -np.inf, rand_y(rs, 5, 90))
    got = check([y, y, y2, y3, y3, rand_y(rs, 3, 5)], [[1, 2], [2, 1], [1], [1], [2], [1, 2]], what="-inf")
    assert list(got[4]) == [0, 1, 1, 1, 0, 0]
    assert list(got[0][0]) == [-1, 0, 0, -1, 1] and got[2][0] == -7.5 and got[3][0] == -7.5
    big = check([y4, holes], [l4, l4[:8]], what="-inf, longer")
    held = big[0][0][40:50]
    assert big[4][0] == 0 and len(set(held)) == 1 and held[0] >= 0 and l4[held[0]] == l4[12]
    assert got[2][1] == -np.inf and got[3][1] == -np.inf and np.all(got[0][1] == -1) and np.all(got[1][1] == -1)


def test_status_2_leaves_the_neighbours_alone():
    import ctc_fast
    rs = np.random.RandomState(5)
    A = 6
    ys = [rand_y(rs, A, T) for T in (20, 20, 20, 20, 20)]
    good = rand_labels(rs, 7, A)
    seqs = [good, [1, 2, A, 3], good, [1, 0, 2], [2 ** 31 - 1]]
    got = check(ys, seqs, what="status 2")
    assert list(got[4]) == [0, 2, 0, 2, 2]
    alone = ctc_fast.align_batch([ys[0], ys[2]], [good, good], total=True)
    for k in range(2):
        assert np.array_equal(got[k][0], alone[k][0]) and np.array_equal(got[k][2], alone[k][1])
    got = check(ys[:2], [[1, 2], [5, 1]], blank=5, what="status 2, blank 5")
    assert list(got[4]) == [0, 2]
    got = check(ys[:1], [[-1]], what="negative label")
    assert list(got[4]) == [2]


def test_layout_and_batch(monkeypatch):
    import torch
    import ctc_fast
    rs = np.random.RandomState(6)
    A = 7
    Ts, Us = [33, 0, 12, 0, 50], [9, 0, 0, 3, 24]
    for dtype in (np.float32, np.float64):
        for blank in (0, A - 1):
            ys = [rand_y(rs, A, T, dtype) for T in Ts]
            seqs = [rand_labels(rs, U, A, blank) for U in Us]
            got = check(ys, seqs, blank=blank, what="mixed %s blank %d" % (dtype.__name__, blank))
            assert list(got[4]) == [0, 0, 0, 1, 0]
            assert got[2][1] == 0.0 and got[3][1] == 0.0
            # independent of the order in the batch, and of the batch
            perm = [3, 0, 4, 2, 1]
            gp = ctc_fast.align_batch([ys[i] for i in perm], [seqs[i] for i in perm], blank=blank, total=True)
            for j, i in enumerate(perm):
                one = ctc_fast.align_batch([ys[i]], [seqs[i]], blank=blank, total=True)
                for k in range(5):
                    assert np.array_equal(gp[k][j], got[k][i]) and np.array_equal(one[k][0], got[k][i]), (i, k)
            # a device tensor with ld > A, read in place
            wide = torch.full((sum(Ts) + 3, A + 5), float("nan"), dtype=torch.float64 if dtype == np.float64 else torch.float32)
            wide[:sum(Ts), :A] = torch.from_numpy(np.concatenate([y.T for y in ys], axis=0))
            dev = wide.cuda()[:, :A]
            assert dev.stride(0) == A + 5
            gd = ctc_fast.align_batch(dev, seqs, lengths=Ts, blank=blank, total=True)
            same_bits(gd, got)
    # repeated label offsets through the C ABI: three utterances share one label row
    _sctc = ctc_fast._sctc
    L = _sctc.lib()
    ys = [rand_y(rs, A, T) for T in (20, 31, 0, 25, 14)]
    l = rand_labels(rs, 6, A)
    Tb = np.array([y.shape[1] for y in ys], np.int32)
    Ub = np.array([6, 6, 0, 6, 0], np.int32)
    fo = np.concatenate([[0], np.cumsum(Tb)[:-1]]).astype(np.int64)
    lo = np.zeros(5, np.int64)
    cfg = _sctc.AlignConfig(5, A, _sctc.F64, 0, A, _sctc.ALIGN_TOTAL, _sctc.i32(Tb), _sctc.i64(fo), _sctc.i32(Ub), _sctc.i64(lo))
    dev = torch.from_numpy(np.concatenate([y.T for y in ys], axis=0)).cuda()
    labels = torch.from_numpy(l).cuda()
    fl = torch.full((int(Tb.sum()),), -7, dtype=torch.int32, device="cuda")
    span = torch.full((18, 2), -7, dtype=torch.int32, device="cuda")
    scores = torch.zeros((5, 2), dtype=torch.float64, device="cuda")
    status = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    rc = L.sctc_ctc_align_batch(ctypes.byref(cfg), dev.data_ptr(), labels.data_ptr(), fl.data_ptr(), span.data_ptr(),
                                scores.data_ptr(), status.data_ptr(), None, 0, _sctc.current_stream_ptr())
    assert rc == 0, L.sctc_last_error()
    with np.errstate(all="ignore"):
        want = am.align_batch(ys, [l, l, [], l, []], total=True)
    fl, span, scores, status = fl.cpu().numpy(), span.cpu().numpy(), scores.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(status, want[4]) and np.array_equal(scores[:, 0], want[2])
    assert np.array_equal(fl, np.concatenate(want[0])) and np.array_equal(span, np.concatenate([s for s in want[1]]))
    assert np.allclose(scores[:, 1], want[3], rtol=TOTAL_RTOL, atol=0)


@pytest.mark.parametrize("T,A", [(50, 5), (300, 33), (700, 40)])
def test_argmax_property(T, A):
    """aligning the collapse of the per-frame argmax reproduces the argmax path"""
    import ctc_fast
    rs = np.random.RandomState(T)
    y = rand_y(rs, A, T)
    best = y.argmax(axis=0)
    srt = np.sort(y, axis=0)
    assert np.all(srt[-1] > srt[-2])            # tie-free
    l = am.collapse(best)
    fl, spans, vit, tot, status = ctc_fast.align_batch([y], [l], total=True)
    assert status[0] == 0
    sym = np.where(fl[0] < 0, 0, np.asarray(l + [0])[fl[0]])
    assert np.array_equal(sym, best)
    run = 0.0
    for t in range(T):
        run = run + y[best[t], t]
    assert vit[0] == run and tot[0] >= vit[0]
    assert_same((fl, spans, vit, tot, status), am.align_batch([y], [l], total=True))


def search_inputs():
    rs = np.random.RandomState(7)
    return [np.asfortranarray(log_softmax_cols(rs.randn(4, T) * 1.5)) for T in (1, 2, 3, 4) for _ in range(6)]


SEARCH_SYMBOLS = {1: "[space]", 2: "a", 3: "e"}
SEARCH_ALPHA, SEARCH_BETA, SEARCH_BEAM = 0.7, 0.3, 128      # 121 prefixes of at most 4 symbols out of 3


def host_sentence_score(y, l, arpa, sym_words, alpha, beta):
    with np.errstate(all="ignore"):
        sc = am.align(y, l, total=True).total
    if arpa is not None:
        ctx = [arpa.bos]
        for c in l:
            sc += alpha * float(arpa.score_ids(ctx, int(sym_words[c])))
            ctx.append(int(sym_words[c]))
    return sc + beta * len(l)


def search_gap_on_the_host():
    """worst |beam_model top score - float64 model score of that hypothesis| over search_inputs(), without and
    with the LM: the float32 rounding of the beam's masses between frames.  Runs on the CPU."""
    import arpa_lm
    arpa = arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_2g.arpa"))
    sw = arpa.symbol_words(SEARCH_SYMBOLS, 4)
    worst = 0.0
    for y in search_inputs():
        for lm in (None, arpa):
            (hyp, score), = beam_model.decode(y, beam=SEARCH_BEAM, alpha=SEARCH_ALPHA, beta=SEARCH_BETA,
                                              lm_row=beam_model.arpa_rows(lm, sw) if lm else None)
            worst = max(worst, abs(score - host_sentence_score(y, list(hyp), lm, sw, SEARCH_ALPHA, SEARCH_BETA)))
    return worst


def test_score_sentences_against_the_search():
    """With a beam that holds every prefix the search's top score is the sentence score of its hypothesis, up
    to the float32 rounding of the beam's masses between frames: measured on the CPU between tests/beam_model.py
    and the float64 model over these inputs (search_gap_on_the_host()) the worst gap is 8.63e-08 (8.7e-08 is asserted); the test
    allows 4 x that = 3.5e-07.  No other sentence scores higher than the top by more than the same margin."""
    import ctc_fast
    ys = search_inputs()
    assert search_gap_on_the_host() <= SEARCH_GAP_MEASURED
    sentences = [list(r) for n in range(5) for r in itertools.product((1, 2, 3), repeat=n)]
    assert len(sentences) == 121 <= SEARCH_BEAM
    dlm = ctc_fast.DecodeLM(os.path.join(GOLDEN, "lm_char_2g.arpa"), SEARCH_SYMBOLS, A=4)
    try:
        for lm in (None, dlm):
            hyps, scores = ctc_fast.decode_beam_batch(ys, beam=SEARCH_BEAM, alpha=SEARCH_ALPHA, beta=SEARCH_BETA, lm=lm)
            own = ctc_fast.score_sentences(ys, hyps, lm=lm, alpha=SEARCH_ALPHA, beta=SEARCH_BETA)
            assert np.all(np.abs(own - scores) <= SEARCH_MARGIN), (own, scores)
            for b, y in enumerate(ys):
                every = ctc_fast.score_sentences([y] * len(sentences), sentences, lm=lm, alpha=SEARCH_ALPHA, beta=SEARCH_BETA)
                assert every.max() <= scores[b] + SEARCH_MARGIN, (b, every.max(), scores[b])
                feasible = [len(s) + repeats(s) <= y.shape[1] for s in sentences]
                assert np.array_equal(np.isfinite(every), feasible)
                want = host_sentence_score(y, sentences[7], dlm.arpa if lm else None, dlm.sym_words, SEARCH_ALPHA, SEARCH_BETA)
                assert every[7] == want or abs(every[7] - want) <= TOTAL_RTOL * abs(want)
    finally:
        dlm.close()


def test_score_sentences_with_the_neural_lm():
    """the DecodeNNLM branch: the LM term is the sum of the float32 rows the search adds, one row per prefix; and
    the unpruned search's top score is the sentence score of its hypothesis up to the float32 rounding of its
    two masses per frame: log-masses below 32 in magnitude are stored to half an ulp of 2^-19 = 2^-20 each"""
    import ctc_fast
    chars = {}
    with open(os.path.join(GOLDEN, "chars.txt")) as f:
        for line in f:
            t, i = line.split()
            chars[int(i)] = t
    dlm = ctc_fast.DecodeNNLM(os.path.join(GOLDEN, "lm_char_nn.npz"), chars, A=4)
    try:
        ys = search_inputs()
        hyps, scores = ctc_fast.decode_beam_batch(ys, beam=SEARCH_BEAM, alpha=SEARCH_ALPHA, beta=SEARCH_BETA, lm=dlm)
        own = ctc_fast.score_sentences(ys, hyps, lm=dlm, alpha=SEARCH_ALPHA, beta=SEARCH_BETA)
        assert np.abs(scores).max() < 32
        for b, (y, h) in enumerate(zip(ys, hyps)):
            with np.errstate(all="ignore"):
                want = am.align(y, h, total=True).total
            for i, c in enumerate(h):
                want += SEARCH_ALPHA * float(dlm.rows([tuple(int(x) for x in h[:i])])[0, int(c)])
            want += SEARCH_BETA * len(h)
            assert abs(own[b] - want) <= TOTAL_RTOL * abs(want), (b, own[b], want)
            assert abs(own[b] - scores[b]) <= y.shape[1] * 2 * 2.0 ** -20, (b, own[b], scores[b])
        assert sum(len(h) for h in hyps) > 0
        lm_only = ctc_fast.lm_sentence_scores([[1, 2, 3], []], dlm)
        assert lm_only[1] == 0.0 and lm_only[0] < 0.0
    finally:
        dlm.close()


def test_decoder_score_and_align():
    from new_decoder import decoder
    import ctc_fast
    import runDecode
    chars = os.path.join(GOLDEN, "chars.txt")
    d = decoder.BeamLMDecoder()
    d.load_chars(chars)
    d.load_lm(os.path.join(GOLDEN, "lm_char_2g.arpa"))
    rs = np.random.RandomState(9)
    y = rand_y(rs, 35, 40)
    hyp, score = d.decode(y, beam=20, alpha=0.5, beta=0.1)
    ids = [d.char_int_map[t] for t in runDecode.tokens(hyp, d.char_int_map)]
    own = d.score(y, ids, alpha=0.5, beta=0.1)
    assert own == ctc_fast.score_sentences([y], [ids], lm=d._device_lm(35), alpha=0.5, beta=0.1)[0]
    # a pruned search keeps a part of the hypothesis's alignments, so it cannot score it higher than the sum over
    # all of them, beyond its float32 masses: half an ulp of a log-mass below 256 (1.5e-5) at each of 40 frames
    assert np.isfinite(own) and score <= own + 40 * 1.5e-5
    fl, spans, vit, status = d.align(y, ids)
    want = am.align(y, ids)
    assert status == 0 and vit == want.viterbi and np.array_equal(fl, want.frame_label) and np.array_equal(spans, want.span)
    assert d.score(y, [1] * 41) == -np.inf


def test_run_decode_ref_scores_and_ctm(tmp_path, capsys):
    import dataLoader as dl
    import runDecode
    import writeLikelihoods as wl
    import ctc_fast
    from new_decoder import decoder
    from nnets import brnnet
    rs = np.random.RandomState(0)
    raw = img = 12
    A = 6
    data = tmp_path / "data"
    data.mkdir()
    names = ["sw02001-a_x_000100-000400", "sw02001-b_x_000500-000900", "plainkey", "u3", "u4"]
    utts = [(k, int(rs.randint(12, 30)), list(rs.randint(1, A, size=3))) for k in names]
    utts[3] = (utts[3][0], 4, [2, 2, 2, 3])             # four frames cannot hold 2 2 2 3: no alignment
    write_shard(data, 1, utts, raw, rs)
    net = brnnet.NNet(img, A, 32, 3, 40, train=False, temporalLayer=2)
    np.random.seed(1)
    net.initParams()
    loader = dl.DataLoader(str(data) + "/", raw, img)
    lik = tmp_path / "lik"
    lik.mkdir()
    wl.writeLogLikes(loader, net, 1, str(lik), writePickle=True)
    chars = tmp_path / "chars.txt"
    chars.write_text("".join(l for l in open(os.path.join(GOLDEN, "chars.txt")).readlines()[:A - 1]))
    lm = os.path.join(GOLDEN, "lm_char_2g.arpa")
    out, reff, ctmf = tmp_path / "hyps.txt", tmp_path / "ref.txt", tmp_path / "hyp.ctm"
    argv = ["--likelihoods", str(lik / "loglikelihoods_1.pk"), "--chars", str(chars), "--alis", str(data / "alis1.txt"),
            "--lm", lm, "--out", str(out), "--beam", "8", "--alpha", "0.5", "--beta", "0.2", "--batch", "2"]
    capsys.readouterr()
    cer = runDecode.main(argv)
    plain_out, plain_hyps = capsys.readouterr().out, out.read_text()
    assert "ref scores" not in plain_out

    cer2 = runDecode.main(argv + ["--ref-scores", str(reff), "--ctm", str(ctmf), "--frame-shift", "0.02"])
    printed = capsys.readouterr().out
    assert cer2 == cer and out.read_text() == plain_hyps
    assert [l for l in printed.splitlines() if not l.startswith("ref scores")] == plain_out.splitlines()

    with open(lik / "loglikelihoods_1.pk", "rb") as f:
        pk = pickle.load(f)
    alis = runDecode.load_alis(str(data / "alis1.txt"), str(chars))
    d = decoder.BeamLMDecoder()
    d.load_chars(str(chars))
    d.load_lm(lm)
    keys = sorted(pk)
    probs = [np.asfortranarray(pk[k], dtype=np.float64) for k in keys]
    hyp = {l.split(" ", 2)[0]: l.rstrip("\n").split(" ", 2)[2] for l in plain_hyps.splitlines()}
    hyp_score = {k: sc for k, (h, sc) in zip(keys, d.decode_batch(probs, 8, 0.5, 0.2))}
    assert all(hyp[k] == h for k, (h, sc) in zip(keys, d.decode_batch(probs, 8, 0.5, 0.2)))
    rows = [l.split() for l in reff.read_text().splitlines()]
    assert [r[0] for r in rows] == keys
    ref_ids = [[d.char_int_map[t] for t in alis[k]] for k in keys]
    want = ctc_fast.score_sentences(probs, ref_ids, lm=d._device_lm(A), alpha=0.5, beta=0.2)
    search_errors = unaligned = 0
    for r, k, w in zip(rows, keys, want):
        assert r[1] == "%.6f" % hyp_score[k] and r[2] == "%.6f" % w
        search_errors += int(w > hyp_score[k])
        unaligned += int(w == -np.inf)
    assert unaligned == 1 and want[keys.index("u3")] == -np.inf
    assert [l for l in printed.splitlines() if l.startswith("ref scores")] == [
        "ref scores of 5 transcripts: %d search errors (refscore > hypscore), 1 without an alignment" % search_errors]

    # the CTM: words in time order within an utterance, starts and durations from the spans
    space = d.char_int_map["[space]"]
    lines = ctmf.read_text().splitlines()
    want_lines = []
    for k, y in zip(keys, probs):
        ids = [d.char_int_map[t] for t in runDecode.tokens(hyp[k], d.char_int_map)]
        res = am.align(y, ids)
        assert res.status == 0
        file_id, chan, offset = runDecode.parse_ctm_key(k)
        runs, cur = [], []
        for u, c in enumerate(ids):
            if c == space:
                runs, cur = runs + ([cur] if cur else []), []
            else:
                cur.append(u)
        runs += [cur] if cur else []
        start_prev = -1
        for run in runs:
            first, last = int(res.span[run[0]][0]), int(res.span[run[-1]][1])
            assert first > start_prev and last >= first
            start_prev = last
            want_lines.append("%s %s %0.2f %0.2f %s" % (file_id, chan, offset + first * 0.02, (last + 1 - first) * 0.02,
                                                       "".join(d.int_char_map[ids[i]] for i in run)))
    assert lines == want_lines and len(lines) > 0
    assert {l.split()[0] for l in lines} <= {"sw02001", "plainkey", "u3", "u4"}
