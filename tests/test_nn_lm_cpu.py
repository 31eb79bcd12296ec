"""CPU-side checks of the neural character LM: the context rule of nn_lm.NNCharLM
against a literal re-reading of clm_decoder2.pyx:52-54, the model file, the exact width padding, the
symbol map, the trainer, and the new C entries' argument checking without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import nn_lm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "lm_char_nn.npz")


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


def int_char_map():
    chars = {}
    with open(os.path.join(GOLDEN, "chars.txt")) as f:
        for l in f:
            t, i = l.split()
            chars[int(i)] = t
    return chars


@pytest.mark.parametrize("K", [1, 2, 8, 19])
def test_context_rule_is_the_reference_s(K):
    lm = M.random_lm(3, 12, K, (32,))
    rs = np.random.RandomState(K)
    lengths = sorted({0, 1, max(K - 1, 0), K, K + 5})
    for n in lengths:
        ids = [int(i) for i in rs.randint(3, lm.V, size=n)]
        want = M.reference_context([lm.tokens[i] for i in ids], K + 1)
        got = [lm.tokens[i] for i in lm.context_ids(ids)]
        assert got == want, (K, n, got, want)
        assert len(got) == K
        if n < K:
            assert got[K - n - 1] == "<s>" and all(t == "<null>" for t in got[:K - n - 1])
        else:
            assert "<s>" not in got and "<null>" not in got


def test_fixture_is_what_its_generator_draws(tmp_path):
    import nn_lm
    lm = nn_lm.NNCharLM.load(FIXTURE)
    assert (lm.V, lm.context, [w.shape[0] for w in lm.weights]) == (37, 8, [64, 64, 37])
    assert os.path.getsize(FIXTURE) < 150 * 1024
    from tests.golden import make_golden_nnlm as g
    chars = [int_char_map()[i] for i in range(1, 35)]
    again = M.random_lm(g.SEED, 37, g.CONTEXT, g.HIDDEN, scale=g.SCALE, chars=chars)
    assert again.tokens == lm.tokens
    for a, b in zip(again.weights + again.biases, lm.weights + lm.biases):
        np.testing.assert_array_equal(a, b)


def test_save_load_round_trip(tmp_path):
    import nn_lm
    lm = M.random_lm(5, 20, 3, (40, 72, 33))
    path = str(tmp_path / "m.npz")
    lm.save(path)
    assert os.path.exists(path)
    back = nn_lm.NNCharLM.load(path)
    assert back.tokens == lm.tokens and back.context == lm.context
    assert (back.null, back.bos, back.eos) == (0, 1, 2)
    for a, b in zip(back.weights + back.biases, lm.weights + lm.biases):
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, b)


def test_bad_models_rejected():
    import nn_lm
    lm = M.random_lm(5, 20, 3, (40,))
    with pytest.raises(ValueError):
        nn_lm.NNCharLM(lm.tokens, 0, lm.weights, lm.biases)
    with pytest.raises(ValueError):
        nn_lm.NNCharLM(lm.tokens, 33, lm.weights, lm.biases)
    with pytest.raises(ValueError):
        nn_lm.NNCharLM(["x%d" % i for i in range(20)], 3, lm.weights, lm.biases)       # no <s> / <null> / </s>
    with pytest.raises(ValueError):
        nn_lm.NNCharLM(lm.tokens, 3, lm.weights[:1], lm.biases[:1])                      # no hidden layer
    with pytest.raises(ValueError):
        nn_lm.NNCharLM(lm.tokens, 3, [lm.weights[0], lm.weights[1][:, :-1]], lm.biases)  # widths do not chain


def test_width_padding_is_exact():
    """hidden widths 40 and 72 padded to 64 and 96: the float64 rows do not move"""
    lm = M.random_lm(6, 50, 5, (40, 72), scale=1.5)
    widths, ws, bs = lm.padded()
    assert list(widths) == [250, 64, 96, 50]
    assert ws[0].shape == (64, 250) and ws[1].shape == (96, 64) and ws[2].shape == (50, 96)
    assert not ws[0][40:].any() and not ws[1][72:].any() and not ws[1][:, 40:].any() and not ws[2][:, 72:].any()
    rs = np.random.RandomState(0)
    for ctx in rs.randint(0, 50, size=(40, 5)):
        a, b = M.forward64(lm, ctx), M.forward64(lm, ctx, ws, bs)
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()


def test_forward_is_the_column_gather():
    """the explicit one-hot product of the restatement equals the sum of K columns"""
    lm = M.random_lm(7, 30, 4, (32,))
    ctx = [5, 0, 29, 1]
    x = M.one_hot_input(lm, ctx)
    assert x.sum() == 4 and x.shape == (120,)
    w0 = lm.weights[0].astype(np.float64)
    cols = sum(w0[:, s * 30 + i] for s, i in enumerate(ctx))
    np.testing.assert_allclose(w0 @ x, cols, rtol=1e-14, atol=1e-14)
    row = M.forward64(lm, ctx)
    assert abs((10.0 ** row).sum() - 1.0) < 1e-12


def test_unmapped_symbol_is_an_error():
    import nn_lm
    lm = nn_lm.NNCharLM.load(FIXTURE)
    chars = int_char_map()
    sw = lm.symbol_words(chars, 35)
    assert sw.dtype == np.int32 and sw[0] == 0 and sorted(sw[1:]) == list(range(3, 37))
    with pytest.raises(ValueError):
        lm.symbol_words(chars, 36)                      # symbol 35 has no token
    other = dict(chars)
    other[7] = "[unseen]"
    with pytest.raises(ValueError):
        lm.symbol_words(other, 35)


def test_rows_provider_feeds_the_beam_model():
    """rows64 is an lm_row provider of the unmodified restatement of the search"""
    import nn_lm
    from tests import beam_model, beam_trace as bt
    lm = nn_lm.NNCharLM.load(FIXTURE)
    sw = lm.symbol_words(int_char_map(), 35)
    rows = M.rows64(lm, sw)
    r = rows((3, 4))
    assert r.shape == (35,) and r[0] == 0.0 and np.all(r[1:] < 0)
    lp = bt.peaked(np.random.RandomState(1), 35, 30)
    with_lm = beam_model.decode(lp, 8, 1.0, 0.5, rows)
    without = beam_model.decode(lp, 8, 0.0, 0.5, rows)
    assert with_lm[0][1] < without[0][1]


def declared_functions():
    src = open(os.path.join(ROOT, "include", "sctc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sctc_[a-z0-9_]+)\s*\(", src)))


NEW = ["sctc_nnlm_create", "sctc_nnlm_destroy", "sctc_nnlm_bytes", "sctc_nnlm_rows",
       "sctc_ctc_nnbeam_workspace_bytes", "sctc_ctc_nnbeam_decode_batch"]


def test_exported_symbols_still_equal_the_header(sctc):
    L = sctc.lib()
    names = declared_functions()
    for n in NEW:
        assert n in names and hasattr(L, n)
    assert sorted(sctc.PROTOTYPES) == names
    assert L.sctc_abi_version() == 6
    assert ctypes.sizeof(sctc.NNBeamConfig) == ctypes.sizeof(sctc.BeamConfig)
    assert sctc.NNBeamConfig.lm.offset == sctc.BeamConfig.lm.offset


def test_new_entries_reject_bad_arguments_without_a_gpu(sctc):
    L = sctc.lib()
    lm = M.random_lm(8, 20, 3, (64, 32))
    widths, ws, bs = lm.padded()

    def create(V=20, K=3, n=3, widths=widths, ws=ws, bs=bs, bos=1, null=0, out=True):
        wp = (ctypes.c_void_p * len(ws))(*[w.ctypes.data if w is not None else None for w in ws])
        bp = (ctypes.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
        h = ctypes.c_void_p()
        wd = np.ascontiguousarray(widths, dtype=np.int32)
        rc = L.sctc_nnlm_create(V, K, n, sctc.i32(wd), wp, bp, bos, null, ctypes.byref(h) if out else None)
        assert not h.value or rc == 0
        return rc, L.sctc_last_error()

    for kw, word in ((dict(V=2), b"vocabulary"), (dict(V=257), b"vocabulary"), (dict(K=0), b"context"),
                     (dict(K=33), b"context"), (dict(n=1), b"weight matrices"), (dict(n=6), b"weight matrices"),
                     (dict(widths=[61, 64, 32, 20]), b"input width"), (dict(widths=[60, 64, 32, 21]), b"output width"),
                     (dict(widths=[60, 40, 32, 20]), b"multiple of 32"), (dict(widths=[60, 64, 4096, 20]), b"multiple of 32"),
                     (dict(ws=[ws[0], None, ws[2]]), b"null parameters"), (dict(bos=20), b"<s>"), (dict(null=-1), b"<null>"),
                     (dict(bos=0, null=0), b"equal"), (dict(out=False), b"null")):
        rc, msg = create(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert L.sctc_nnlm_destroy(None) == 0 and L.sctc_nnlm_bytes(None) == 0
    assert L.sctc_nnlm_rows(None, None, 4, None, None) == -1 and b"null LM" in L.sctc_last_error()
    T = np.array([5], dtype=np.int32)
    off = np.zeros(1, dtype=np.int64)
    sw = np.zeros(8, dtype=np.int32)
    cfg = sctc.NNBeamConfig(1, 8, sctc.F32, 4, 1, 0, 8, sctc.i32(T), sctc.i64(off), 1.0, 0.0, None, sctc.i32(sw))
    assert L.sctc_ctc_nnbeam_workspace_bytes(ctypes.byref(cfg)) == 0 and b"null LM" in L.sctc_last_error()
    assert L.sctc_ctc_nnbeam_workspace_bytes(None) == 0 and b"null config" in L.sctc_last_error()
    assert L.sctc_ctc_nnbeam_decode_batch(ctypes.byref(cfg), None, None, None, None, None, 0, None) == -1
    assert L.sctc_ctc_nnbeam_decode_batch(None, None, None, None, None, None, 0, None) == -1
    import ctc_fast
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(sctc.SctcError):
            ctc_fast.DecodeNNLM(FIXTURE, int_char_map(), 35)
    with pytest.raises(ValueError):
        ctc_fast.DecodeNNLM(FIXTURE, int_char_map(), 36)        # the symbol map is checked before the device
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch([np.zeros((8, 3))], lm=object())


def alignment_text(path):
    """the golden shard's alignments as lines of character tokens"""
    chars = int_char_map()
    with open(os.path.join(GOLDEN, "shard", "alis1.txt")) as f, open(path, "w") as out:
        for l in f:
            out.write(" ".join(chars[int(i)] for i in l.split()[1:]) + "\n")


def test_trainer_output_loads_and_beats_uniform(tmp_path):
    import nn_lm
    from tools import train_char_nnlm as tr
    text, out = str(tmp_path / "text.txt"), str(tmp_path / "lm.npz")
    alignment_text(text)
    tr.main(["--text", text, "--chars", os.path.join(GOLDEN, "chars.txt"), "--out", out, "--context", "4",
             "--hidden", "24", "40", "--steps", "30", "--batch", "8", "--lr", "0.01"])
    lm = nn_lm.NNCharLM.load(out)
    assert (lm.V, lm.context, [w.shape[0] for w in lm.weights]) == (37, 4, [24, 40, 37])
    assert list(lm.padded()[0]) == [148, 32, 64, 37]
    X, Y = tr.examples(lm.tokens, 4, [l.strip() for l in open(text)])
    assert X.shape == (15, 4) and list(X[0]) == [0, 0, 0, 1] and Y[-1] == lm.eos
    score = -np.mean([M.forward64(lm, x)[y] for x, y in zip(X, Y)])
    print("trained LM: %.3f log10 units per token, uniform %.3f" % (score, np.log10(lm.V)))
    assert score < np.log10(lm.V)
