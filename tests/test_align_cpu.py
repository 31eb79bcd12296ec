"""CPU checks of the CTC forced alignment: the NumPy model of the contract
(tests/align_model.py) against exhaustive enumeration and against the C oracle's ctc_loss, its tie and
-inf rules on hand-worked lattices, the argument errors of the C ABI (no device needed) and the CTM
helpers of runDecode.py."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import align_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


def label_rows(max_len=3, symbols=(1, 2)):
    return [list(r) for n in range(max_len + 1) for r in itertools.product(symbols, repeat=n)]


def log_softmax_cols(z):
    z = z - z.max(axis=0, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=0, keepdims=True))


def check_path(y, labels, res, blank=0):
    """the path of a status-0 result is a path of the label row, its score is the Viterbi score, and the
    spans are the first and last frame of every label"""
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[1]
    fl = res.frame_label
    sym = [blank if u < 0 else int(labels[u]) for u in fl]
    assert am.collapse(sym, blank) == [int(c) for c in labels]
    lab = [u for u in fl if u >= 0]
    assert all(b - a in (0, 1) for a, b in zip(lab, lab[1:])) and (not lab or (lab[0] == 0 and lab[-1] == len(labels) - 1))
    sc = 0.0
    for t in range(T):
        sc = sc + y[sym[t], t]
    assert sc == res.viterbi
    for u in range(len(labels)):
        fr = np.nonzero(fl == u)[0]
        assert tuple(res.span[u]) == (fr[0], fr[-1]) and np.all(np.diff(fr) == 1)


def test_model_against_enumeration():
    rs = np.random.RandomState(11)
    rows = label_rows()
    assert len(rows) == 15
    n_bad = 0
    for T in range(1, 6):
        for variant in ("dense", "holes"):
            y = log_softmax_cols(rs.randn(3, T) * 2.0)
            if variant == "holes":
                with np.errstate(all="ignore"):
                    y = np.where(rs.rand(3, T) < 0.25, -np.inf, y)
            for l in rows:
                want_v, want_t = am.enumerate_paths(y, l)
                got = am.align(y, l, total=True)
                if want_v == -np.inf:
                    n_bad += 1
                    assert got.status == 1 and got.viterbi == -np.inf and got.total == -np.inf
                    assert np.all(got.frame_label == -1) and np.all(got.span == -1)
                    continue
                assert got.status == 0
                assert got.viterbi == want_v, (T, l)                        # bit-equal: a chain of additions
                assert abs(got.total - want_t) <= 1e-12 * max(1.0, abs(want_t)), (T, l, got.total, want_t)
                assert got.total >= got.viterbi - 1e-12
                check_path(y, l, got)
                assert np.isnan(am.align(y, l).total)
    assert n_bad > 20      # T < U + repeats and cut lattices were among the cases


def test_model_edge_statuses():
    y = np.zeros((3, 0))
    r = am.align(y, [], total=True)
    assert r.status == 0 and r.viterbi == 0.0 and r.total == 0.0 and r.frame_label.shape == (0,)
    assert am.align(y, [1]).status == 1
    y = log_softmax_cols(np.random.RandomState(2).randn(3, 4))
    for bad in ([3], [1, -1], [0], [1, 0, 2]):
        r = am.align(y, bad, total=True)
        assert r.status == 2 and r.viterbi == -np.inf and np.all(r.frame_label == -1) and r.span.shape == (len(bad), 2)
    r = am.align(y, [1, 2], blank=2)
    assert r.status == 2
    r = am.align(y, [0, 1], blank=2, total=True)
    want_v, want_t = am.enumerate_paths(y, [0, 1], blank=2)
    assert r.status == 0 and r.viterbi == want_v and abs(r.total - want_t) < 1e-12
    # float32 inputs are widened exactly
    y32 = y.astype(np.float32)
    assert am.align(y32, [1, 2]).viterbi == am.align(y32.astype(np.float64), [1, 2]).viterbi


def test_model_total_against_the_oracle_loss():
    from oracle import ctc as octc
    rs = np.random.RandomState(5)
    T, U, A = 200, 40, 33
    p = np.exp(log_softmax_cols(rs.randn(A, T)))
    p = np.asfortranarray(p / p.sum(axis=0, keepdims=True))
    seq = rs.randint(1, A, size=U).astype(np.int32)
    seq[5] = seq[4]                 # a repeat
    cost, _, skip = octc.ctc_loss(p, seq)
    assert not skip
    got = am.align(np.log(p), seq, total=True)
    assert got.status == 0
    assert abs(got.total + cost) <= 1e-11 * abs(cost), (got.total, cost)
    assert got.viterbi <= got.total
    check_path(np.log(p), seq, got)


def test_model_minus_inf_frames():
    y = np.full((3, 5), -np.inf)
    forced = [0, 1, 1, 0, 2]        # one finite symbol per frame: the path is forced
    for t, c in enumerate(forced):
        y[c, t] = -0.5 * (t + 1)
    r = am.align(y, [1, 2], total=True)
    assert r.status == 0 and list(r.frame_label) == [-1, 0, 0, -1, 1]
    assert r.viterbi == -7.5 and r.total == -7.5 and r.span.tolist() == [[1, 2], [4, 4]]
    assert am.align(y, [2, 1]).status == 1
    y2 = log_softmax_cols(np.random.RandomState(3).randn(3, 5))
    y2[:, 2] = -np.inf              # a frame of all -inf
    assert am.align(y2, [1], total=True).status == 1
    y3 = log_softmax_cols(np.random.RandomState(4).randn(3, 6))
    y3[0, 3] = y3[1, 3] = -np.inf   # the lattice of [1] is cut in the middle: only symbol 2 survives frame 3
    r = am.align(y3, [1], total=True)
    assert r.status == 1 and r.total == -np.inf
    assert am.align(y3, [2]).status == 0


def test_model_tie_rule_on_an_all_equal_lattice():
    # every complete path scores T * -1.0; "stay" wins every tie and the end prefers S-1, so the path leaves each
    # state as late as it can: it sits in the final blank and reaches it by the earliest frames
    y = np.full((3, 6), -1.0)
    r = am.align(y, [1, 2], total=True)
    assert r.status == 0 and r.viterbi == -6.0
    assert list(r.frame_label) == [0, 1, -1, -1, -1, -1]      # states 1, 3 (skip), then the last blank
    r = am.align(y, [1, 1])
    assert list(r.frame_label) == [0, -1, 1, -1, -1, -1]      # no skip between equal labels: 1, 2, 3, 4, 4, 4
    r = am.align(y, [1, 2, 1])
    assert list(r.frame_label) == [0, 1, 2, -1, -1, -1]
    r = am.align(np.full((3, 3), -1.0), [1, 2, 1])            # T = U: the single path, it ends in S-2
    assert list(r.frame_label) == [0, 1, 2] and r.span.tolist() == [[0, 0], [1, 1], [2, 2]]
    r = am.align(np.full((3, 2), -1.0), [1])                  # ending tie between S-1 and S-2: S-1
    assert list(r.frame_label) == [0, -1]
    y = np.full((3, 2), -1.0)
    y[0, 1] = -1.5                                            # now S-2 is strictly better
    assert list(am.align(y, [1]).frame_label) == [0, 0]


def test_model_speed_at_the_wide_threshold():
    import time
    rs = np.random.RandomState(1)
    y = log_softmax_cols(rs.randn(5, 1100))
    seq = rs.randint(1, 5, size=256)
    t0 = time.time()
    r = am.align(y, seq, total=True)
    assert r.status == 0 and time.time() - t0 < 1.5     # about 0.15 s on an idle core


def align_cfg(sctc, T_b, U_b, A=5, dtype=0, blank=0, ld=None, flags=0, frame_off=None, label_off=None):
    Tb, Ub = np.array(T_b, dtype=np.int32), np.array(U_b, dtype=np.int32)
    fo = np.array(frame_off if frame_off is not None else np.concatenate([[0], np.cumsum(Tb)[:-1]]), dtype=np.int64)
    lo = np.array(label_off if label_off is not None else np.concatenate([[0], np.cumsum(Ub)[:-1]]), dtype=np.int64)
    cfg = sctc.AlignConfig(len(Tb), A, dtype, blank, A if ld is None else ld, flags, sctc.i32(Tb), sctc.i64(fo),
                           sctc.i32(Ub), sctc.i64(lo))
    return cfg, (Tb, Ub, fo, lo)        # the arrays must outlive the call


def test_argument_errors_need_no_gpu(sctc):
    L = sctc.lib()
    n = ctypes.c_size_t(7)
    fake = ctypes.c_void_p(4096)        # never dereferenced: every call below fails before the device is touched

    def run(cfg, ws=0, outs=(fake,) * 6):
        return L.sctc_ctc_align_batch(ctypes.byref(cfg) if cfg is not None else None, *outs, None, ws, None)

    assert L.sctc_ctc_align_workspace_bytes(None, ctypes.byref(n)) == -1 and n.value == 0
    assert run(None) == -1
    cfg, keep = align_cfg(sctc, [100, 7], [10, 0])
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), None) == -1
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0 and n.value == 0   # on chip
    import ctc_fast
    plan = ctc_fast.align_plan(10)
    assert plan == {"path": "wave", "spl": 1, "nl": 64, "fpw": 16, "lds_frames": 4096, "stage_frames": 1024}
    cfg, keep = align_cfg(sctc, [plan["lds_frames"], plan["lds_frames"] + 1], [10, 10])
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert n.value == 257 * 64 * 4      # the second utterance alone: 4097 frames, 16 to a word, 64 lanes
    assert run(cfg, ws=n.value - 1) == -3 and b"workspace" in L.sctc_last_error()
    cfg, keep = align_cfg(sctc, [8000], [800])
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert n.value == 4000 * 256 * 4    # wide: 1601 states on 256 threads, two frames to a word
    for kw in ({"A": 0}, {"dtype": 2}, {"blank": 5}, {"blank": -1}, {"ld": 4}, {"flags": 2}):
        cfg, keep = align_cfg(sctc, [5], [2], **kw)
        assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1, kw
        assert run(cfg) == -1, kw
    for T_b, U_b in (([5, -1], [1, 1]), ([5, 5], [1, 4096]), ([5, 5], [-1, 1])):
        cfg, keep = align_cfg(sctc, T_b, U_b, frame_off=[0, 5], label_off=[0, 1])
        assert run(cfg) == -1
    assert b"outside 0..4095" in L.sctc_last_error()
    cfg, keep = align_cfg(sctc, [5, 5], [1, 4095])
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    cfg, keep = align_cfg(sctc, [5, 5], [1, 1], frame_off=[0, -5])
    assert run(cfg) == -1
    cfg, keep = align_cfg(sctc, [5, 5], [1, 1], label_off=[-1, 0])
    assert run(cfg) == -1 and b"negative offset" in L.sctc_last_error()
    cfg, keep = align_cfg(sctc, [5], [1])
    cfg.B = -1
    assert run(cfg) == -1
    cfg = sctc.AlignConfig(1, 5, 0, 0, 5, 0, None, None, None, None)
    assert run(cfg) == -1
    # missing output pointers
    cfg, keep = align_cfg(sctc, [5], [2])
    for hole in range(6):
        outs = tuple(None if i == hole else fake for i in range(6))
        assert run(cfg, outs=outs) == -1, hole
    # B == 0: nothing to do, nothing launched, no pointer looked at
    cfg = sctc.AlignConfig(0, 5, 0, 0, 5, 0, None, None, None, None)
    assert run(cfg, outs=(None,) * 6) == 0
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0 and n.value == 0
    # the Python surface checks before it needs a device
    y = np.zeros((5, 4))
    with pytest.raises(ValueError):
        ctc_fast.align_batch([y], [[1], [2]])
    with pytest.raises(ValueError):
        ctc_fast.align_batch([y], [np.ones(4096, np.int32)])
    with pytest.raises(ValueError):
        ctc_fast.align_batch([y], [[1.5]])
    with pytest.raises(ValueError):
        ctc_fast.align_batch([y], [[1]], blank=5)


def test_forced_path_is_checked(sctc, monkeypatch):
    L = sctc.lib()
    n = ctypes.c_size_t(0)
    cfg, keep = align_cfg(sctc, [600], [256])
    monkeypatch.setenv("SCTC_ALIGN_PATH", "wave")
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1     # 513 states
    monkeypatch.setenv("SCTC_ALIGN_PATH", "lds")
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1
    monkeypatch.setenv("SCTC_ALIGN_PATH", "wide")
    cfg, keep = align_cfg(sctc, [4096], [10])
    assert L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == 0
    assert n.value == 2048 * 64 * 4     # forced wide: eight states a thread, two frames to a word


def test_no_cpu_fallback(sctc):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctc_fast
    with pytest.raises(sctc.SctcError):
        ctc_fast.align_batch([np.zeros((3, 4))], [[1]])
    with pytest.raises(sctc.SctcError):
        ctc_fast.score_sentences([np.zeros((3, 4))], [[1]])


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    fields = ["B", "A", "dtype", "blank", "ld", "flags", "T_b", "frame_off", "U_b", "label_off"]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
        'int main(void){printf("%zu ' + "%zu " * len(fields) + '%d\\n", sizeof(sctc_align_config),'
        + "".join(" offsetof(sctc_align_config, %s)," % f for f in fields) + ' SCTC_ALIGN_TOTAL); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    C = sctc.AlignConfig
    assert got == [ctypes.sizeof(C)] + [getattr(C, f).offset for f in fields] + [sctc.ALIGN_TOTAL]


def test_ctm_words_of_an_unaligned_hypothesis():
    import runDecode
    assert runDecode.ctm_words([1, 2], np.full((2, 2), -1, np.int32), 3, {1: "a", 2: "b"}) == []


def test_ctm_key_parser_and_line_format():
    import runDecode
    assert runDecode.parse_ctm_key("sw02001-a_x_000098-001156") == ("sw02001", "A", 0.98)
    assert runDecode.parse_ctm_key("sw04390-b_y_012345-012999") == ("sw04390", "B", 123.45)
    for key in ("utt3", "a_b", "sw02001-a_x_000098", "sw02001-a_x_12-ab", "a_b_1-2-3"):
        assert runDecode.parse_ctm_key(key) == (key, "A", 0.0)
    chars = {1: "a", 2: "b", 3: "[space]", 4: "c"}
    ids = [3, 1, 2, 3, 3, 4, 3, 2]
    spans = [[0, 0], [2, 3], [4, 4], [6, 6], [7, 9], [10, 12], [13, 13], [15, 20]]
    words = runDecode.ctm_words(ids, spans, 3, chars)
    assert words == [("ab", 2, 4), ("c", 10, 12), ("b", 15, 20)]
    assert runDecode.ctm_words([], np.zeros((0, 2), np.int32), 3, chars) == []
    assert runDecode.ctm_words([1, 4], [[1, 1], [5, 6]], None, chars) == [("ac", 1, 6)]
    lines = runDecode.ctm_lines("sw02001-a_x_000098-001156", words, 0.01)
    assert lines == ["sw02001 A 1.00 0.03 ab\n", "sw02001 A 1.08 0.03 c\n", "sw02001 A 1.13 0.06 b\n"]
    assert runDecode.ctm_lines("utt3", words[:1], 0.02) == ["utt3 A 0.04 0.06 ab\n"]
