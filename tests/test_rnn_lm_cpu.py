"""CPU-side checks of the recurrent character LM: the protocol of
clm_decoder2.pyx:43-80 driven by a stub model against nn_lm.RNNCharLM, the model file and its
``kind``, the exact width padding, rejections, a lane-by-lane emulation of the index arithmetic of
csrc/rnnlm_dev.h, the trainer, and the new C entries' argument checking without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import nn_lm_model as FF
from tests import rnn_lm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "lm_char_rnn.npz")


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


# ---- the protocol of the reference's search -----------------------------------------------------

class StubModel(object):
    """stands where clm_decoder2's ``lm`` stands: it is handed token strings and the previous state
    (or None), notes both, and answers with the float64 model"""

    def __init__(self, lm):
        self.lm, self.calls = lm, []

    def run(self, tokens, prev_h0):
        self.calls.append((list(tokens), None if prev_h0 is None else prev_h0.copy()))
        h = prev_h0
        for t in tokens:
            h = M.step64(self.lm, h, self.lm.vocab[t])
        return M.row64(self.lm, h), h


def score_prefix(stub, tokens_of_prefix, cache):
    """what clm_decoder2.pyx:43-80 asks of its model for one prefix (a tuple of token strings): with a
    cached state of the prefix without its last token, that token alone and the state; otherwise --
    the empty prefix -- <s> and no state.  The new state is cached under the prefix."""
    P = tuple(tokens_of_prefix)
    if len(P) > 0 and P[:-1] in cache:
        row, h = stub.run(P[-1:], cache[P[:-1]])
    else:
        assert len(P) == 0, "the search asks for a prefix only after the prefix it extends"
        row, h = stub.run(["<s>"], None)
    cache[P] = h
    return row


def test_protocol_is_the_reference_s():
    import nn_lm
    lm = nn_lm.RNNCharLM.load(FIXTURE)
    assert M.spectral_norm(lm.Wh) < 1
    stub, cache = StubModel(lm), {}
    rs = np.random.RandomState(2)
    seq = [lm.tokens[i] for i in rs.randint(3, lm.V, size=12)]
    for n in range(len(seq) + 1):
        row = score_prefix(stub, seq[:n], cache)
        tokens, prev = stub.calls[-1]
        if n == 0:
            assert tokens == ["<s>"] and prev is None
        else:
            assert tokens == [seq[n - 1]]
            np.testing.assert_array_equal(prev, cache[tuple(seq[:n - 1])])
        h, want = M.forward64(lm, [lm.vocab[t] for t in seq[:n]])
        np.testing.assert_allclose(cache[tuple(seq[:n])], h, rtol=0, atol=1e-13)
        np.testing.assert_allclose(row, want, rtol=0, atol=1e-12)
        assert abs((10.0 ** row).sum() - 1.0) < 1e-12
    assert "<null>" not in [t for c in stub.calls for t in c[0]]
    # the provider of the beam model walks the same chain
    sw = lm.symbol_words(int_char_map(), 35)
    inv = {int(sw[c]): c for c in range(1, 35)}
    P = tuple(inv[lm.vocab[t]] for t in seq)
    r = M.rows64(lm, sw)(P)
    assert r.shape == (35,) and r[0] == 0.0
    np.testing.assert_allclose(r[1:], M.forward64(lm, [lm.vocab[t] for t in seq])[1][sw[1:]], rtol=0, atol=1e-12)


def test_fixture_is_what_its_generator_draws():
    import nn_lm
    lm = nn_lm.RNNCharLM.load(FIXTURE)
    assert (lm.V, lm.H) == (37, 64) and os.path.getsize(FIXTURE) < 64 * 1024
    from tests.golden import make_golden_rnnlm as g
    chars = [int_char_map()[i] for i in range(1, 35)]
    again = M.random_lm(g.SEED, 37, g.HIDDEN, scale=g.SCALE, rho=g.RHO, chars=chars)
    assert again.tokens == lm.tokens
    for name in ("Wx", "Wh", "bh", "Wo", "bo"):
        np.testing.assert_array_equal(getattr(again, name), getattr(lm, name))
    rows = np.stack([M.forward64(lm, rs)[1] for rs in np.random.RandomState(0).randint(3, 37, size=(20, 6))])
    assert rows.max() - rows.min() > 3          # several decades


@pytest.mark.parametrize("H,Hp", [(40, 64), (64, 64), (33, 64), (544, 544)])
def test_width_padding_is_exact(H, Hp):
    lm = M.random_lm(6, 50, H)
    got_Hp, Wx, Wh, bh, Wo = lm.padded()
    assert got_Hp == Hp and Wx.shape == (Hp, 50) and Wh.shape == (Hp, Hp) and bh.shape == (Hp,) and Wo.shape == (50, Hp)
    assert not Wx[H:].any() and not Wh[H:].any() and not Wh[:, H:].any() and not bh[H:].any() and not Wo[:, H:].any()
    ids = [int(i) for i in np.random.RandomState(0).randint(0, 50, size=9)]
    h, row = M.forward64(lm, ids)
    hp = M.state64(lm, ids, Wx=Wx, Wh=Wh, bh=bh)
    np.testing.assert_array_equal(hp[H:], 0.0)
    # a padded product adds zeros only; the matrix product may sum a wider row in another order
    assert np.abs(hp[:H] - h).max() <= 1e-13 * np.abs(h).max()
    assert np.abs(M.row64(lm, hp, Wo=Wo) - row).max() <= 1e-13 * np.abs(row).max()


def test_save_load_and_kind_dispatch(tmp_path):
    import nn_lm
    lm = M.random_lm(5, 20, 40)
    path = str(tmp_path / "r.npz")
    lm.save(path)
    with np.load(path) as z:
        assert str(z["kind"]) == "rnn"
    for back in (nn_lm.RNNCharLM.load(path), nn_lm.load(path)):
        assert isinstance(back, nn_lm.RNNCharLM) and back.tokens == lm.tokens
        assert (back.null, back.bos, back.eos) == (0, 1, 2)
        for name in ("Wx", "Wh", "bh", "Wo", "bo"):
            assert getattr(back, name).dtype == np.float32
            np.testing.assert_array_equal(getattr(back, name), getattr(lm, name))
    # a file without `kind` stays the feed-forward model, for both loaders
    ff = FF.random_lm(5, 20, 3, (40,))
    ffpath = str(tmp_path / "f.npz")
    ff.save(ffpath)
    with np.load(ffpath) as z:
        assert "kind" not in z.files
    assert isinstance(nn_lm.load(ffpath), nn_lm.NNCharLM) and isinstance(nn_lm.NNCharLM.load(ffpath), nn_lm.NNCharLM)
    assert isinstance(nn_lm.load(os.path.join(GOLDEN, "lm_char_nn.npz")), nn_lm.NNCharLM)
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM.load(ffpath)
    bad = str(tmp_path / "b.npz")
    with open(bad, "wb") as f:
        np.savez(f, kind=np.array("ngram"), tokens=np.array(lm.tokens))
    with pytest.raises(ValueError):
        nn_lm.load(bad)
    from new_decoder import decoder
    d = decoder.BeamLMDecoder()
    d.load_lm(path)
    assert isinstance(d.lm, nn_lm.RNNCharLM)
    d.load_lm(ffpath)
    assert isinstance(d.lm, nn_lm.NNCharLM)


def test_bad_models_rejected():
    import nn_lm
    lm = M.random_lm(5, 20, 40)
    a = (lm.Wx, lm.Wh, lm.bh, lm.Wo, lm.bo)
    nn_lm.RNNCharLM(lm.tokens, *a)
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(["x%d" % i for i in range(20)], *a)                       # no <s> / <null> / </s>
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens[:2], lm.Wx[:, :2], lm.Wh, lm.bh, lm.Wo[:2], lm.bo[:2])   # V < 3
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(["<null>", "<s>", "</s>"] + ["t%d" % i for i in range(254)], np.zeros((4, 257)),
                        np.zeros((4, 4)), np.zeros(4), np.zeros((257, 4)), np.zeros(257))   # V > 256
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens, np.zeros((2049, 20)), np.zeros((2049, 2049)), np.zeros(2049), np.zeros((20, 2049)),
                        lm.bo)                                                   # H > 2048
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens, np.zeros((0, 20)), np.zeros((0, 0)), np.zeros(0), np.zeros((20, 0)), lm.bo)
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens, lm.Wx, lm.Wh[:, :-1], lm.bh, lm.Wo, lm.bo)
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens, lm.Wx, lm.Wh, lm.bh[:-1], lm.Wo, lm.bo)
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens, lm.Wx, lm.Wh, lm.bh, lm.Wo[:-1], lm.bo)
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens, lm.Wx, lm.Wh, lm.bh, lm.Wo, lm.bo[:-1])
    with pytest.raises(ValueError):
        nn_lm.RNNCharLM(lm.tokens[:-1] + [lm.tokens[3]], *a)                      # a token twice
    fix = nn_lm.RNNCharLM.load(FIXTURE)
    chars = int_char_map()
    sw = fix.symbol_words(chars, 35)
    assert sw.dtype == np.int32 and sw[0] == 0 and sorted(sw[1:]) == list(range(3, 37))
    with pytest.raises(ValueError):
        fix.symbol_words(chars, 36)                       # symbol 35 has no token
    other = dict(chars)
    other[7] = "[unseen]"
    with pytest.raises(ValueError):
        fix.symbol_words(other, 35)


# ---- the index arithmetic of rnnlm_dev.h, lane by lane -------------------------------------------

TILE = 32


def repack_quads(W, rows_padded):
    """W [n][k] -> X[k / 4][n][4] with zero rows up to rows_padded, as sctc_rnnlm_create stores Wh and Wo"""
    n, k = W.shape
    out = np.zeros((k // 4, rows_padded, 4), dtype=W.dtype)
    for u in range(n):
        for kk in range(k):
            out[kk >> 2, u, kk & 3] = W[u, kk]
    return out


def mfma_32x32x2(a, b, acc):
    """v_mfma_f32_32x32x2_f32 on 64 lanes: lane l holds A[l % 32][l / 32] and
    B[l / 32][l % 32]; register r of lane (n = l % 32, g = l / 32) holds D[8 (r / 4) + 4 g + r % 4][n]"""
    A = np.stack([a[:32], a[32:]], axis=1)          # [m][k]
    B = np.stack([b[:32], b[32:]], axis=0)          # [k][n]
    lane, r = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
    n, g = lane & 31, lane >> 5
    m = 8 * (r // 4) + 4 * g + r % 4
    return (acc + A[m, 0] * B[0, n]) + A[m, 1] * B[1, n]          # every (lane, register) on its own


def emulate_tile(lm_padded, ids, src, dst, cnt, sin, n_out):
    """rnnlm_tile's recurrent step in float64, with the kernel's layouts and lane maps: returns sout"""
    H, Wx, Wh, bh = lm_padded
    wx_cols = np.ascontiguousarray(Wx.T.astype(np.float64))                    # [V][H]
    whq = repack_quads(Wh.astype(np.float64), H)
    pre = np.zeros((H // 4, TILE, 4))
    par = np.zeros((H // 4, TILE, 4))
    # pre-activation and the gather: wave e % 4 takes slot e, lane q % 64 the quad q
    for e in range(TILE):
        for q in range(H // 4):
            if e < cnt:
                pre[q, e] = bh[4 * q:4 * q + 4].astype(np.float64) + wx_cols[ids[e], 4 * q:4 * q + 4]
                if sin is not None:
                    par[q, e] = sin[src[e], 4 * q:4 * q + 4]
    sout = np.full((n_out, H), np.nan)
    TN = 4 if H >= 512 else 1
    nt, nj = H >> 5, H >> 3
    lanes = np.arange(64)
    e_of, g_of = lanes & 31, lanes >> 5
    for wv in range(4):
        for t0 in range(wv * TN, nt, 4 * TN):
            for i in range(TN):
                tile = t0 + i
                if tile >= nt:
                    continue
                acc = np.zeros((64, 16))
                for rq in range(4):
                    acc[:, 4 * rq:4 * rq + 4] = pre[tile * 8 + rq * 2 + g_of, e_of]      # the accumulator init
                for j in range(nj):
                    aq = whq[2 * j + g_of, tile * 32 + e_of]            # [64][4]: unit tile * 32 + e, quad 2j + g
                    bq = par[2 * j + g_of, e_of]                        # [64][4]: slot e, quad 2j + g
                    for c in range(4):
                        acc = mfma_32x32x2(aq[:, c], bq[:, c], acc)
                acc = np.maximum(acc, 0.0)
                for lane in range(64):
                    e, g = lane & 31, lane >> 5
                    for rq in range(4):
                        v = acc[lane, 4 * rq:4 * rq + 4]
                        pre[tile * 8 + rq * 2 + g, e] = v                                 # the next layer's operand
                        if e < cnt:
                            sout[dst[e], tile * 32 + rq * 8 + g * 4:tile * 32 + rq * 8 + g * 4 + 4] = v   # the scatter
    return sout, pre


@pytest.mark.parametrize("H,Hp,cnt", [(64, 64, 32), (40, 64, 7), (512, 512, 3), (544, 544, 2)])
def test_lane_emulation_reproduces_float64(H, Hp, cnt):
    lm = M.random_lm(30 + H, 24, H)
    assert M.spectral_norm(lm.Wh) < 1
    got_Hp, Wx, Wh, bh, _ = lm.padded()
    assert got_Hp == Hp
    rs = np.random.RandomState(H)
    n_in, n_out = cnt + 3, cnt + 2
    parents = [[int(i) for i in rs.randint(3, 24, size=rs.randint(0, 4))] for _ in range(n_in)]
    sin = np.zeros((n_in, Hp))
    for r, P in enumerate(parents):
        sin[r, :H] = M.state64(lm, P)
    ids = [int(i) for i in rs.randint(0, 24, size=cnt)]
    src = [int(i) for i in rs.randint(0, n_in, size=cnt)]
    dst = [int(i) for i in rs.permutation(n_out)[:cnt]]
    sout, pre = emulate_tile((Hp, Wx, Wh, bh), ids, src, dst, cnt, sin, n_out)
    worst = 0.0
    for e in range(cnt):
        want = M.step64(lm, sin[src[e], :H], ids[e])
        scale = max(1.0, np.abs(want).max())
        worst = max(worst, np.abs(sout[dst[e], :H] - want).max() / scale)
        np.testing.assert_array_equal(sout[dst[e], H:], 0.0)
        # the operand of the output layer is the same state in the quad layout
        np.testing.assert_array_equal(pre[:, e].reshape(-1), sout[dst[e]])
    print("lane emulation H %d -> %d, %d slots: max |emulation - float64| / scale = %.3g" % (H, Hp, cnt, worst))
    assert worst <= 1e-14
    untouched = [r for r in range(n_out) if r not in dst]
    assert np.isnan(sout[untouched]).all() and not pre[:, cnt:].any()
    # the zero state goes the same way and leaves the pre-activation's relu
    zero, _ = emulate_tile((Hp, Wx, Wh, bh), [lm.bos], [0], [0], 1, None, 1)
    np.testing.assert_array_equal(zero[0, :H], M.step64(lm, None, lm.bos))


def test_forward32_is_close_to_float64():
    lm = M.random_lm(3, 30, 48)
    rs = np.random.RandomState(1)
    prefixes = [tuple(int(i) for i in rs.randint(3, 30, size=n)) for n in (0, 1, 5, 20, 20)]
    s32, r32 = M.forward32(lm, prefixes)
    assert s32.dtype == np.float32 and r32.dtype == np.float64
    for P, s, r in zip(prefixes, s32, r32):
        h, row = M.forward64(lm, P)
        assert np.abs(s - h).max() < 1e-4 and np.abs(r - row).max() < 1e-4
    assert np.abs(r32 - np.stack([M.forward64(lm, P)[1] for P in prefixes])).max() > 0


# ---- the C entries without a GPU -------------------------------------------------------------------

NEW = ["sctc_rnnlm_create", "sctc_rnnlm_destroy", "sctc_rnnlm_bytes", "sctc_rnnlm_step",
       "sctc_ctc_rnnbeam_workspace_bytes", "sctc_ctc_rnnbeam_decode_batch"]


def test_new_entries_exported_and_reject_bad_arguments_without_a_gpu(sctc):
    L = sctc.lib()
    for n in NEW:
        assert n in sctc.PROTOTYPES and hasattr(L, n)
    assert L.sctc_abi_version() == 6
    assert ctypes.sizeof(sctc.RNNBeamConfig) == ctypes.sizeof(sctc.NNBeamConfig)
    assert sctc.RNNBeamConfig.lm.offset == sctc.NNBeamConfig.lm.offset
    lm = M.random_lm(8, 20, 64)
    Hp, Wx, Wh, bh, Wo = lm.padded()

    def create(V=20, H=Hp, ptrs=(Wx, Wh, bh, Wo, lm.bo), bos=1, out=True):
        h = ctypes.c_void_p()
        rc = L.sctc_rnnlm_create(V, H, *[p.ctypes.data if p is not None else None for p in ptrs], bos,
                                 ctypes.byref(h) if out else None)
        assert not h.value or rc == 0
        return rc, L.sctc_last_error()

    for kw, word in ((dict(V=2), b"vocabulary"), (dict(V=257), b"vocabulary"), (dict(H=40), b"multiple of 32"),
                     (dict(H=0), b"multiple of 32"), (dict(H=2080), b"multiple of 32"),
                     (dict(ptrs=(Wx, None, bh, Wo, lm.bo)), b"null parameters"), (dict(bos=20), b"<s>"),
                     (dict(bos=-1), b"<s>"), (dict(out=False), b"null")):
        rc, msg = create(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert L.sctc_rnnlm_destroy(None) == 0 and L.sctc_rnnlm_bytes(None) == 0
    assert L.sctc_rnnlm_step(None, None, None, 4, None, None, None) == -1 and b"null LM" in L.sctc_last_error()
    T = np.array([5], dtype=np.int32)
    off = np.zeros(1, dtype=np.int64)
    sw = np.zeros(8, dtype=np.int32)
    cfg = sctc.RNNBeamConfig(1, 8, sctc.F32, 4, 1, 0, 8, sctc.i32(T), sctc.i64(off), 1.0, 0.0, None, sctc.i32(sw))
    assert L.sctc_ctc_rnnbeam_workspace_bytes(ctypes.byref(cfg)) == 0 and b"null LM" in L.sctc_last_error()
    assert L.sctc_ctc_rnnbeam_workspace_bytes(None) == 0 and b"null config" in L.sctc_last_error()
    assert L.sctc_ctc_rnnbeam_decode_batch(ctypes.byref(cfg), None, None, None, None, None, 0, None) == -1
    assert L.sctc_ctc_rnnbeam_decode_batch(None, None, None, None, None, None, 0, None) == -1
    import ctc_fast
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(sctc.SctcError):
            ctc_fast.DecodeRNNLM(FIXTURE, int_char_map(), 35)
    with pytest.raises(ValueError):
        ctc_fast.DecodeRNNLM(FIXTURE, int_char_map(), 36)        # the symbol map is checked before the device
    with pytest.raises(ValueError):
        ctc_fast.DecodeRNNLM(FIXTURE, np.full(35, 37, dtype=np.int32))


# ---- the trainer -----------------------------------------------------------------------------------

def test_trainer_writes_a_recurrent_model(tmp_path):
    import nn_lm
    from tools import train_char_nnlm as tr
    chars = int_char_map()
    text, out = str(tmp_path / "text.txt"), str(tmp_path / "lm.npz")
    with open(os.path.join(GOLDEN, "shard", "alis1.txt")) as f, open(text, "w") as o:
        lines = [" ".join(chars[int(i)] for i in l.split()[1:]) for l in f]
        o.write("\n".join((lines * 3)[:12]) + "\n")
    tr.main(["--text", text, "--chars", os.path.join(GOLDEN, "chars.txt"), "--out", out, "--rnn", "--hidden", "24",
             "--steps", "5", "--batch", "4", "--lr", "0.01"])
    lm = nn_lm.load(out)
    assert isinstance(lm, nn_lm.RNNCharLM) and (lm.V, lm.H) == (37, 24) and lm.padded()[0] == 32
    toks = lines[0].split()
    for n in (0, 1, len(toks)):
        row = M.forward64(lm, [lm.vocab[t] for t in toks[:n]])[1]
        assert abs((10.0 ** row).sum() - 1.0) < 1e-12
    data = tr.sentences(lm.tokens, lines[:1])
    assert data[0][0][0] == lm.bos and data[0][1][-1] == lm.eos and len(data[0][0]) == len(toks) + 1
