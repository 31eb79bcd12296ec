"""GPU checks of batched best-path decoding and of the device logarithm (csrc/ctc_bestpath.hip).
Everything is compared against the NumPy model of the contract (tests/bestpath_model.py): ids, lengths and spans
equal; the score bit-equal on dyadic-grid inputs (every order of the sum is exact) and within 1e-13 * sum|v| on
random log-softmax inputs (T <= 1000 float64 additions of either order: T * 2^-53 * sum|v| < 1.2e-13 * sum|v|)."""
import ctypes
import os

import numpy as np
import pytest

from tests import bestpath_model as bm

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-13
MAPS = [None, "lane", "wave"]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def cf():
    import ctc_fast
    return ctc_fast


@pytest.fixture
def force_map():
    def force(m):
        if m is None:
            os.environ.pop("SCTC_BESTPATH_MAP", None)
        else:
            os.environ["SCTC_BESTPATH_MAP"] = m
    yield force
    os.environ.pop("SCTC_BESTPATH_MAP", None)


def check_batch(cf, rows_list, drop, exact, **kw):
    """decode the batch, compare every utterance with the model; returns the device results"""
    hyps, spans, scores = cf.decode_best_path_batch([np.asfortranarray(r.T) for r in rows_list], blank=None, drop=drop,
                                                    spans=True, scores=True, **kw)
    assert len(hyps) == len(spans) == len(rows_list) and scores.shape == (len(rows_list),)
    for b, rows in enumerate(rows_list):
        best, ids, sp, score = bm.decode(rows, drop)
        assert hyps[b].dtype == np.int32 and np.array_equal(hyps[b], ids), (b, rows.shape)
        assert spans[b].shape == sp.shape and np.array_equal(spans[b], sp), (b, rows.shape)
        if exact or np.isinf(score):
            assert scores[b] == score, (b, scores[b], score)
        else:
            assert abs(scores[b] - score) <= SCORE_RTOL * bm.abs_sum(rows, best), (b, scores[b], score)
    return hyps, spans, scores


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MAPS)
def test_every_length_and_alphabet(cf, force_map, m, dtype):
    force_map(m)
    rs = np.random.RandomState(7)
    for A in bm.A_SWEEP + bm.A_SWITCH:
        drop = (0,) if A > 1 else ()
        lengths = bm.T_SWEEP if A in bm.A_SWEEP else bm.T_SWITCH
        grid = [bm.plant(bm.random_path(T, A, rs), A, dtype, rs) for T in lengths]
        check_batch(cf, grid, drop, exact=True)
        soft = [bm.log_softmax_rows(T, A, dtype, rs) for T in lengths]
        check_batch(cf, soft, drop, exact=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MAPS)
@pytest.mark.parametrize("A", [10, 70])
def test_planted_paths(cf, force_map, A, m, dtype):
    force_map(m)
    rs = np.random.RandomState(11)
    cases = bm.planted_paths()
    for drop in sorted(set(d for _, d in cases.values())):
        names = [n for n in sorted(cases) if cases[n][1] == drop]
        rows = [bm.plant(cases[n][0], A, dtype, rs) for n in names]
        hyps, spans, _ = check_batch(cf, rows, drop, exact=True)
        got = dict(zip(names, zip(hyps, spans)))
        if "one_symbol" in got:
            T = len(cases["one_symbol"][0])
            assert got["one_symbol"][0].tolist() == [5] and got["one_symbol"][1].tolist() == [[0, T - 1]]
            assert len(got["new_symbol_every_frame"][0]) == len(cases["new_symbol_every_frame"][0])
            assert len(got["all_blank"][0]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MAPS)
def test_ties_and_rows_of_minus_infinity(cf, force_map, m, dtype):
    force_map(m)
    for A in (2, 33, 300):
        trows, want = bm.tie_rows(A, dtype)
        ids, _, _ = check_batch(cf, [trows, bm.neg_inf_rows(A, dtype)], (), exact=True)
        assert ids[0].tolist() == [r[0] for r in bm.runs(want)]
        assert ids[1][0] == 0


@pytest.mark.parametrize("m", MAPS)
def test_wide_alphabet_with_a_row_stride(cf, force_map, m):
    import torch
    force_map(m)
    rs = np.random.RandomState(5)
    A, ld, Ts = 300, 304, [130, 0, 257, 64]
    rows = [bm.plant(bm.random_path(T, A, rs), A, np.float32, rs) for T in Ts]
    host = np.full((sum(Ts), ld), 9.0, dtype=np.float32)        # columns A..ld would win every arg-max
    host[:, :A] = np.concatenate(rows)
    dev = torch.from_numpy(host).cuda()
    hyps, spans, scores = cf.decode_best_path_batch(dev[:, :A], lengths=Ts, blank=0, drop=(), spans=True, scores=True)
    for b, r in enumerate(rows):
        best, ids, sp, score = bm.decode(r, (0,))
        assert np.array_equal(hyps[b], ids) and np.array_equal(spans[b], sp) and scores[b] == score


def test_mixed_lengths_and_order(cf):
    rs = np.random.RandomState(3)
    A, Ts = 33, [0, 1, 513, 0, 300, 1]
    rows = [bm.plant(bm.random_path(T, A, rs, mean_run=1.5), A, np.float32, rs) for T in Ts]
    h0, s0, c0 = check_batch(cf, rows, (0,), exact=True)
    assert len(h0[0]) == 0 and c0[0] == 0.0 and s0[0].shape == (0, 2)
    perm = [2, 5, 0, 4, 1, 3]
    h1, s1, c1 = check_batch(cf, [rows[i] for i in perm], (0,), exact=True)
    for j, i in enumerate(perm):
        assert np.array_equal(h1[j], h0[i]) and np.array_equal(s1[j], s0[i]) and c1[j] == c0[i]


def test_three_hundred_short_utterances(cf):
    rs = np.random.RandomState(4)
    A = 33
    rows = [bm.plant(bm.random_path(int(T), A, rs, mean_run=2.0), A, np.float32, rs) for T in rs.randint(0, 40, size=300)]
    check_batch(cf, rows, bm.REF_DROP, exact=True)


def test_device_tensor_input_and_device_output(cf):
    import torch
    rs = np.random.RandomState(6)
    A, Ts = 33, [70, 300, 5]
    rows = [bm.log_softmax_rows(T, A, np.float64, rs) for T in Ts]
    host_form = cf.decode_best_path_batch([np.asfortranarray(r.T) for r in rows], spans=True, scores=True)
    dev = torch.from_numpy(np.concatenate(rows)).cuda()
    with pytest.raises(ValueError):
        cf.decode_best_path_batch(dev)
    tensor_form = cf.decode_best_path_batch(dev, lengths=Ts, spans=True, scores=True)
    ids, lens, spans, scores = cf.decode_best_path_batch(dev, lengths=Ts, spans=True, scores=True, device=True)
    assert ids.is_cuda and lens.is_cuda and spans.is_cuda and scores.is_cuda
    assert ids.dtype == torch.int32 and tuple(spans.shape) == (sum(Ts), 2) and scores.dtype == torch.float64
    ids_h, lens_h, spans_h = ids.cpu().numpy(), lens.cpu().numpy(), spans.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(Ts)])
    for b in range(len(Ts)):
        _, want_ids, want_sp, _ = bm.decode(rows[b], (0, 1, 2, 8))
        for hyps, sp, sc in (host_form, tensor_form):
            assert np.array_equal(hyps[b], want_ids) and np.array_equal(sp[b], want_sp)
            assert sc[b] == host_form[2][b]
        assert lens_h[b] == len(want_ids)
        assert np.array_equal(ids_h[off[b]:off[b] + lens_h[b]], want_ids)
        assert np.array_equal(spans_h[off[b]:off[b] + lens_h[b]], want_sp)
    assert np.array_equal(scores.cpu().numpy(), host_form[2])
    only_ids = cf.decode_best_path_batch(dev, lengths=Ts, device=True)
    assert only_ids[2] is None and only_ids[3] is None and np.array_equal(only_ids[0].cpu().numpy()[:5], ids_h[:5])


def test_equals_decode_best_path_per_utterance(cf):
    rs = np.random.RandomState(8)
    A = 12
    probs = []
    for T in (1, 40, 300):
        p = np.exp(bm.log_softmax_rows(T, A, np.float64, rs))
        probs.append(np.asfortranarray(p.T))
    for blank in (0, 5):
        hyps, aligns = cf.decode_best_path_batch(probs, blank=blank)
        for b, p in enumerate(probs):
            hyp, align = cf.decode_best_path(p, blank)
            assert hyps[b].tolist() == hyp and aligns[b].tolist() == align
            assert hyps[b].dtype == np.int32 and aligns[b].dtype == np.int32


def test_argmax_decoder_batch_equals_decode(cf):
    from new_decoder import decoder
    rs = np.random.RandomState(9)
    A = 12
    dec = decoder.ArgmaxDecoder()
    dec.int_char_map = {i: chr(ord("a") + i) for i in range(A)}
    probs = [np.asfortranarray(bm.log_softmax_rows(T, A, np.float64, rs).T) for T in (1, 2, 77, 400)]
    got = dec.decode_batch(probs)
    for p, (hyp, score) in zip(probs, got):
        want_hyp, want_score = dec.decode(p)
        assert hyp == want_hyp
        assert abs(score - want_score) <= 1e-13 * abs(want_score)


def test_log_rows(cf, capsys):
    import torch
    import _sctc
    rs = np.random.RandomState(10)
    rows, A, ld = 517, 33, 40
    p = rs.rand(rows, ld).astype(np.float32)
    p[:, :A] /= p[:, :A].sum(axis=1, keepdims=True)
    p[0, :4] = [0.0, np.float32(1e-45), 1.0, np.finfo(np.float32).tiny]
    p[:, A:] = -7.0                                               # guards: never read, never written
    want = bm.log_rows(p[:, :A])
    worst = 0
    # contiguous, out of place
    dev = torch.from_numpy(np.ascontiguousarray(p[:, :A])).cuda()
    out = cf.log_rows(dev)
    got = out.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), p[:, :A])            # the input is left alone
    assert np.isneginf(got[0, 0]) and got[0, 2] == 0.0 and np.isfinite(got[0, 1]) and got[0, 1] < -103
    worst = max(worst, int(bm.ulp_distance(got, want).max()))
    # ld > A, in place
    wide = torch.from_numpy(p).cuda()
    view = wide[:, :A]
    assert cf.log_rows(view, out=view) is view
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, A:], p[:, A:])                   # the guards are untouched
    worst = max(worst, int(bm.ulp_distance(got[:, :A], want).max()))
    # the C entry itself, out of place with a stride
    src = torch.from_numpy(p).cuda()
    dst = torch.full((rows, ld), 5.0, dtype=torch.float32, device="cuda")
    rc = _sctc.lib().sctc_log_rows(src.data_ptr(), dst.data_ptr(), rows, A, ld, _sctc.current_stream_ptr())
    assert rc == 0
    got = dst.cpu().numpy()
    assert (got[:, A:] == 5.0).all()
    worst = max(worst, int(bm.ulp_distance(got[:, :A], want).max()))
    with capsys.disabled():
        print("sctc_log_rows: worst distance to the float64 logarithm rounded to float32: %d ulp" % worst)
    assert worst <= 1


def test_c_entry_with_null_spans_and_scores(cf):
    import torch
    import _sctc
    rs = np.random.RandomState(12)
    A, Ts = 33, [100, 20]
    rows = [bm.plant(bm.random_path(T, A, rs), A, np.float32, rs) for T in Ts]
    dev = torch.from_numpy(np.concatenate(rows)).cuda()
    Tb = np.array(Ts, dtype=np.int32)
    off = np.array([0, 100], dtype=np.int64)
    cfg = _sctc.BestPathConfig(2, A, _sctc.F32, 1, (ctypes.c_int32 * 16)(0), A, _sctc.i32(Tb), _sctc.i64(off))
    ids = torch.full((120,), -1, dtype=torch.int32, device="cuda")
    lens = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    rc = _sctc.lib().sctc_ctc_bestpath_batch(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(), None, None,
                                             _sctc.current_stream_ptr())
    assert rc == 0
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    for b, o in enumerate(off):
        want = bm.decode(rows[b], (0,))[1]
        assert lens[b] == len(want) and np.array_equal(ids[o:o + lens[b]], want)
        assert (ids[o + lens[b]:o + Ts[b]] == -1).all()           # nothing is written behind the labels
