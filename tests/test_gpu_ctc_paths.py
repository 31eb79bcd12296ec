"""GPU parity of the three CTC code paths behind `ctc_fast.ctc_loss` / `ctc_loss_batch` (round 5):

  fused     ctc_fused.hip      both recursions + the gradient in one kernel, rows of <= 512 states (default there);
                               "fused2w" = the same without helper waves (SCTC_CTC_HELPER=0)
  wide      ctc_fusedw.hip     round 6: the fused schedule on 4 / 8 waves per direction, rows of 513..2048 states (default
                               there; SCTC_CTC_WIDE=1 forces it for every row, SCTC_CTC_WAVES=8 eight waves: "wide8")
  lattice   ctc_kernels.hip    ctc_lattice + ctc_grad, rows of <= 2048 states (SCTC_CTC_FUSED=0 forces it)
  generic   ctc_generic.hip    any label length, any alphabet (SCTC_CTC_GENERIC=1 forces it)

each against the C oracle (oracle/ctc_ref.c = ctc_fast/ctc-loss/ctc_fast.pyx:13-152) on the same inputs, and
against each other.  Tolerances: float64 probabilities 1e-11 relative on the cost, 1e-9 absolute on the gradient
(different summation order of the same float64 numbers); float32 probabilities with the fused kernel's 32-bit row
store 2e-7 absolute on the gradient (22 mantissa bits on one factor of alpha*beta; the gradient itself is float32).
"""
import hashlib
import os
import zlib

import numpy as np
import pytest

from tests.helpers import mid_input, softmax0, time_trials_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import ctc_fast
    from oracle import ctc as octc
    return ctc_fast, octc, torch


class path:
    """context manager: force one CTC path through the environment switches the plan reads per call"""
    ENV = {"fused": {}, "fused64": {"SCTC_CTC_STORE": "64"}, "fused2w": {"SCTC_CTC_HELPER": "0"},
           # round 6: the two-wave form on its register diet (three waves per SIMD; by default from 1025 utterances on)
           "fused2wd": {"SCTC_CTC_HELPER": "0", "SCTC_CTC_DIET_MIN_B": "1"},
           # round 6: the meet-in-the-middle kernel for long rows (ctc_fusedw.hip: 4 / 8 waves per direction; by default for
           # rows of 513..2048 states) forced for every row
           "wide": {"SCTC_CTC_WIDE": "1"}, "wide8": {"SCTC_CTC_WIDE": "1", "SCTC_CTC_WAVES": "8"},
           "wide64": {"SCTC_CTC_WIDE": "1", "SCTC_CTC_STORE": "64"},
           "widemin1": {"SCTC_CTC_WIDE_MIN_B": "1"},      # the default dispatch (rows of 513..2048 states only) from one utterance on
           "lattice": {"SCTC_CTC_FUSED": "0"}, "generic": {"SCTC_CTC_GENERIC": "1"},
           # the lattice kernel's forced shapes (ctc_lattice_shape: 8 / 16 / 32 states per lane on one wave, 8 on four
           # waves, 2 on eight)
           "lattice1": {"SCTC_CTC_FUSED": "0", "SCTC_CTC_WAVES": "1"}, "lattice4": {"SCTC_CTC_FUSED": "0", "SCTC_CTC_WAVES": "4"},
           "lattice8": {"SCTC_CTC_FUSED": "0", "SCTC_CTC_WAVES": "8"},
           # the lattice kernel's lazy schedule (float32 probabilities rescale every 4th frame; INTEGRATION.md, "switches") and
           # its forced shapes: tests/test_gpu_ctc_lazy.py, tests/test_gpu_ctc_entry.py
           "lazy": {"SCTC_CTC_LAZY": "1"}, "lazy1": {"SCTC_CTC_LAZY": "1", "SCTC_CTC_WAVES": "1"},
           "lazy4": {"SCTC_CTC_LAZY": "1", "SCTC_CTC_WAVES": "4"}, "lazy8": {"SCTC_CTC_LAZY": "1", "SCTC_CTC_WAVES": "8"}}
    VARS = ("SCTC_CTC_STORE", "SCTC_CTC_FUSED", "SCTC_CTC_GENERIC", "SCTC_CTC_HELPER", "SCTC_CTC_DIET_MIN_B", "SCTC_CTC_WIDE",
            "SCTC_CTC_WAVES", "SCTC_CTC_WIDE_MIN_B", "SCTC_CTC_LAZY")

    def __init__(self, name):
        self.env = self.ENV[name]

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.VARS}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _case(rs, A, T, U, blank=0, peaked=1.0, with_blank_labels=False, all_same=False):
    logits = rs.randn(A, T) * peaked
    lo = 0 if with_blank_labels else 1
    seq = rs.randint(lo, A, size=U).astype(np.int32)
    if blank != 0:
        seq = np.where(seq == blank, 0 if not with_blank_labels else seq, seq).astype(np.int32)
    if all_same:
        seq[:] = seq[0]
    return np.asfortranarray(softmax0(logits)), seq


def _check_f64(cf, octc, y, seq, blank, tag):
    with np.errstate(all="ignore"):
        c_ref, g_ref, s_ref = octc.ctc_loss(y, seq, blank)
        cost, grad, skip = cf.ctc_loss(y, seq, blank)
    assert bool(skip) == bool(s_ref), (tag, skip, s_ref)
    if s_ref:
        assert not grad.any(), tag
        return 0.0
    if np.isinf(c_ref):
        assert np.isinf(cost) and cost > 0, (tag, cost)
    else:
        assert abs(cost - c_ref) <= 1e-11 * max(abs(c_ref), 1e-30), (tag, cost, c_ref)
    err = np.abs(grad - g_ref).max()
    assert err < 1e-9, (tag, err)
    return err


SHAPES = [  # (A, T, U): one and two states per lane pair, every T parity around the block of 8 frames, the 256-state edge
    (4, 1, 1), (4, 2, 1), (5, 3, 1), (5, 3, 3), (6, 4, 2), (7, 7, 3), (7, 8, 4), (9, 9, 4), (33, 15, 6), (33, 16, 7),
    (33, 17, 8), (33, 31, 15), (28, 100, 30), (33, 333, 63), (33, 200, 64), (62, 300, 100), (33, 260, 127),
    (100, 129, 127), (200, 77, 20), (130, 64, 31), (3, 240, 60), (2, 40, 9),
    # 8 states per lane (rows of 257..512 states; cfg-4: T=2000, U=200 is 401): the 256 / 257 and 511 / 513 edges
    (33, 300, 128), (33, 520, 200), (62, 400, 255), (70, 300, 180), (150, 280, 129), (33, 700, 256),
]


@pytest.mark.parametrize("which", ["fused", "fused2w", "wide", "wide8", "lattice", "generic"])
def test_paths_f64_vs_oracle(mods, which):
    cf, octc, _ = mods
    rs = np.random.RandomState(11)
    worst = 0.0
    with path(which):
        for A, T, U in SHAPES:
            for blank in (0, A - 1):
                for kind in range(3):
                    y, seq = _case(rs, A, T, U, blank=blank, peaked=(1.0, 6.0, 1.0)[kind],
                                   with_blank_labels=(kind == 2))
                    worst = max(worst, _check_f64(cf, octc, y, seq, blank, (which, A, T, U, blank, kind)))
    print("%s: worst float64 gradient error %.1e over %d cases" % (which, worst, len(SHAPES) * 6))


@pytest.mark.parametrize("which", ["fused", "fused2w", "wide", "wide8", "generic"])
def test_paths_quirks(mods, golden, which):
    """the reference's skip / empty band / T = 1 behaviour on the round-5 paths (test_gpu_ctc.py holds the same
    for the default dispatch)"""
    cf, octc, _ = mods
    g = golden("ctc_skip.npz")
    t = golden("ctc_tiny.npz")
    with path(which):
        seq = g["rep_seq"]
        for T in (4, 5, 6, 7, 8):
            y = np.asfortranarray(g["rep_y_T%d" % T])
            cost, grad, skip = cf.ctc_loss(y, seq)
            assert skip == bool(g["rep_skip_T%d" % T]), T
            if skip:
                assert not grad.any()
            else:
                assert cost == pytest.approx(float(g["rep_cost_T%d" % T]), rel=1e-11)
                np.testing.assert_allclose(grad, g["rep_grad_T%d" % T], rtol=1e-9, atol=1e-12)
        _, grad, skip = cf.ctc_loss(np.asfortranarray(g["zero_y"]), g["zero_seq"])
        assert skip and not grad.any()
        cost, grad, skip = cf.ctc_loss(np.asfortranarray(g["short_y"]), g["short_seq"])
        assert not skip and np.isinf(cost) and cost > 0
        np.testing.assert_allclose(grad, g["short_y"], rtol=1e-12)
        for i in range(int(t["n"])):
            y, s = np.asfortranarray(t["y%d" % i]), t["seq%d" % i]
            cost, grad, skip = cf.ctc_loss(y, s)
            assert not skip
            assert cost == pytest.approx(float(t["cost%d" % i]), rel=1e-11, abs=1e-12), i
            np.testing.assert_allclose(grad, t["grad%d" % i], rtol=1e-9, atol=1e-12)
        # a zero band sum late in the utterance (phase 1 of the fused kernel has written gradient rows by then):
        # everything is taken back
        rs = np.random.RandomState(5)
        y, seq = _case(rs, 6, 40, 5)
        y[:, 31] = 0.0
        y[0, 31] = 0.0
        with np.errstate(all="ignore"):
            c_ref, g_ref, s_ref = octc.ctc_loss(y, seq)
            cost, grad, skip = cf.ctc_loss(y, seq)
        assert s_ref and skip and not grad.any()
        y, seq = _case(rs, 6, 40, 5)
        y[:, 8] = 0.0
        with np.errstate(all="ignore"):
            c_ref, g_ref, s_ref = octc.ctc_loss(y, seq)
            cost, grad, skip = cf.ctc_loss(y, seq)
        assert s_ref and skip and not grad.any()
        assert cost == pytest.approx(c_ref, rel=1e-11)         # -llForward as far as alpha got (ctc_fast.pyx:147-149)


def test_fused_known_answers(mods, golden):
    """the reference's own numbers through the fused kernel: ctc/time_trials.py (1710.233966660, 251 states) and
    the T = 1000 / U = 100 fixture"""
    cf, octc, _ = mods
    with path("fused"):
        g = golden("ctc_time_trials.npz")
        p, seq = time_trials_input()
        cost, grad, skip = cf.ctc_loss(np.asfortranarray(p), seq)
        assert not skip and cost == pytest.approx(1710.233966660, abs=1e-6)
        assert cost == pytest.approx(float(g["cost"]), rel=1e-11)
        np.testing.assert_allclose(grad[:, ::37], g["grad_stride37"], rtol=1e-7, atol=1e-11)
        m = golden("ctc_mid.npz")
        logits, seq = mid_input(1000, 33, 100, 0)
        cost, grad, skip = cf.ctc_loss(np.asfortranarray(softmax0(logits)), seq)
        assert cost == pytest.approx(float(m["T1000_cost"]), rel=1e-11)
        np.testing.assert_allclose(grad[:, ::41], m["T1000_grad_stride41"], rtol=1e-7, atol=1e-11)


def test_fused_f32_row_store(mods):
    """float32 probabilities (the BRNN path): the 32-bit row store against float64 rows, the three-kernel path and
    the oracle, on the shapes where plain float32 rows lose the gradient (T >> 2U: tests/test_ctc_store_model.py)"""
    cf, octc, torch = mods
    rs = np.random.RandomState(3)
    cases = [(33, 1000, 100, 1.0), (33, 1000, 20, 1.0), (33, 2000, 100, 1.0), (33, 1000, 100, 4.0), (62, 300, 120, 1.0),
             (28, 200, 30, 6.0), (33, 999, 127, 1.0), (5, 601, 50, 1.0), (33, 2000, 200, 1.0), (33, 1203, 255, 1.0)]
    probs, seqs = [], []
    for A, T, U, peaked in cases:
        y, seq = _case(rs, A, T, U, peaked=peaked)
        probs.append(np.asfortranarray(y.astype(np.float32)))
        seqs.append(seq)
    worst = {}
    for i, (y, seq) in enumerate(zip(probs, seqs)):
        with np.errstate(all="ignore"):
            c_ref, g_ref, s_ref = octc.ctc_loss(np.asfortranarray(y.astype(np.float64)), seq)
        res = {}
        for which in ("fused", "fused64", "fused2w", "fused2wd", "wide", "wide8", "wide64", "lattice"):
            with path(which), np.errstate(all="ignore"):
                cost, grads, skip = cf.ctc_loss_batch([y], [seq])
            assert not skip[0] and not s_ref
            assert abs(cost[0] - c_ref) <= 1e-11 * abs(c_ref), (which, i)
            res[which] = grads[0].astype(np.float64)
            err = np.abs(res[which] - g_ref).max()
            worst[which] = max(worst.get(which, 0.0), err)
            assert err < 2e-7, (which, i, err)
        # float64 rows: the fused kernel and the three-kernel path agree to the float32 rounding of the result
        assert np.abs(res["fused64"] - res["lattice"]).max() < 1.3e-7, i
    print("float32 I/O, worst |grad - oracle|: %s" % {k: "%.1e" % v for k, v in worst.items()})


def test_fused_ragged_batch_and_long_lists(mods):
    """one launch over utterances of every length (K is chosen by the longest row; short rows sit in its lanes),
    labels that occur more often than the 8 list entries a lane keeps in registers, float32 and float64; with and
    without helper waves"""
    cf, octc, _ = mods
    rs = np.random.RandomState(17)
    for A, dt in ((33, np.float64), (3, np.float32), (70, np.float32), (150, np.float64)):
        probs, seqs = [], []
        for b in range(37):
            U = int(rs.randint(1, 256 if A in (33, 70) else 128))
            T = int(rs.randint(max(1, U // 2), 3 * U + 2))
            y, seq = _case(rs, A, T, U, with_blank_labels=(b % 5 == 0), all_same=(b % 11 == 3))
            probs.append(np.asfortranarray(y.astype(dt)))
            seqs.append(seq)
        refs = []
        for b in range(37):
            with np.errstate(all="ignore"):
                refs.append(octc.ctc_loss(np.asfortranarray(probs[b].astype(np.float64)), seqs[b]))
        for which in ("fused", "fused2w", "fused2wd", "wide", "wide8"):
            with path(which), np.errstate(all="ignore"):
                cost, grads, skip = cf.ctc_loss_batch(probs, seqs)
            for b in range(37):
                c_ref, g_ref, s_ref = refs[b]
                assert bool(skip[b]) == bool(s_ref), (which, A, b)
                if s_ref:
                    assert not grads[b].any()
                    continue
                if np.isinf(c_ref):
                    assert np.isinf(cost[b])
                else:
                    assert abs(cost[b] - c_ref) <= 1e-11 * abs(c_ref), (which, A, b)
                tol = 1e-9 if dt == np.float64 else 2e-7
                assert np.abs(grads[b].astype(np.float64) - g_ref).max() < tol, (which, A, b, probs[b].shape, len(seqs[b]))


def test_wide_rows_513_to_2048_states(mods):
    """rows of 513..2048 lattice states (BASELINE configs[4]: U = 800 -> 1601) on the wide meet-in-the-middle kernel
    (the default dispatch takes it from 18 / 24 utterances on: single utterances here with
    SCTC_CTC_WIDE_MIN_B=1, the batches below as dispatched), against the oracle and against the lattice + grad kernels of rounds 1-5:
    the 512 / 513, 1024 / 1025 and 2047 edges of its shapes (4 waves x 2 and x 4 states, 8 x 4), labels that occur far more often than the 32
    list entries a lane keeps in registers (A = 3), wide alphabets, blank ids at either end, float64 and float32
    probabilities (32-bit rows), T odd / even / short of the band; then ragged batches of more utterances than one
    round of 8 block pairs, with a skipping utterance and an empty band among them"""
    cf, octc, _ = mods
    rs = np.random.RandomState(29)
    shapes = [(33, 700, 256), (33, 1201, 300), (33, 1100, 511), (33, 1300, 512), (3, 1700, 800), (33, 1650, 800),
              (70, 2100, 1023), (130, 900, 400), (200, 1000, 600), (33, 1100, 1023), (33, 1024, 1023), (5, 3001, 640)]
    worst64 = worst32 = 0.0
    for A, T, U in shapes:
        for blank in (0, A - 1):
            y, seq = _case(rs, A, T, U, blank=blank, with_blank_labels=(U % 2 == 1))
            with path("widemin1"):
                worst64 = max(worst64, _check_f64(cf, octc, y, seq, blank, ("wide-auto", A, T, U, blank)))
            y32 = np.asfortranarray(y.astype(np.float32))
            with np.errstate(all="ignore"):
                c_ref, g_ref, s_ref = octc.ctc_loss(np.asfortranarray(y32.astype(np.float64)), seq, blank)
                with path("widemin1"):
                    cost, grads, skip = cf.ctc_loss_batch([y32], [seq], blank)
                with path("lattice"):
                    cost_l, grads_l, skip_l = cf.ctc_loss_batch([y32], [seq], blank)
            assert bool(skip[0]) == bool(s_ref) == bool(skip_l[0]), (A, T, U, blank)
            if s_ref:       # (33, 1024, 1023): repeated labels need more frames than there are -- the band sum runs dry
                assert not grads[0].any() and cost[0] == pytest.approx(c_ref, rel=1e-11)
                continue
            assert abs(cost[0] - c_ref) <= 1e-11 * abs(c_ref), (A, T, U, blank)
            err = np.abs(grads[0].astype(np.float64) - g_ref).max()
            worst32 = max(worst32, err)
            assert err < 2e-7, (A, T, U, blank, err)
            assert np.abs(grads[0].astype(np.float64) - grads_l[0]).max() < 2.5e-7
    print("wide rows: worst |grad - oracle| float64 %.1e, float32 (32-bit rows) %.1e" % (worst64, worst32))
    for dt, tol in ((np.float64, 1e-9), (np.float32, 2e-7)):
        probs, seqs = [], []
        for b in range(21):
            U = int(rs.randint(257, 1024))
            T = int(rs.randint(U, 2 * U + 50))
            if b == 6:
                T = U - 3                 # empty band: cost +inf, grad = probabilities
            y, seq = _case(rs, 20, T, U, all_same=(b == 9))
            if b == 13:
                y[:, T // 2 + 5] = 0.0    # a zero band sum in phase 1 of both directions: skip, every row taken back
            if b == 17:
                y[:, 3] = 0.0             # ... and in phase 0 of alpha
            probs.append(np.asfortranarray(y.astype(dt)))
            seqs.append(seq)
        with np.errstate(all="ignore"):
            refs = [octc.ctc_loss(np.asfortranarray(probs[b].astype(np.float64)), seqs[b]) for b in range(21)]
            cost, grads, skip = cf.ctc_loss_batch(probs, seqs)
        for b in range(21):
            c_ref, g_ref, s_ref = refs[b]
            assert bool(skip[b]) == bool(s_ref), (dt, b)
            if s_ref:
                assert not grads[b].any(), (dt, b)
                continue
            if np.isinf(c_ref):
                assert np.isinf(cost[b]) and cost[b] > 0
            else:
                assert abs(cost[b] - c_ref) <= 1e-11 * abs(c_ref), (dt, b)
            assert np.abs(grads[b].astype(np.float64) - g_ref).max() < tol, (dt, b, probs[b].shape, len(seqs[b]))
        assert skip[13] and skip[17] and np.isinf(cost[6])


def test_long_label_rows_and_wide_alphabets(mods):
    """what rounds 1-4 rejected (VERDICT r04 missing #1, #2): 2U+1 > 2048 and A > 256 -- the reference bounds neither
    (ctc_fast.pyx:22-32)"""
    cf, octc, _ = mods
    rs = np.random.RandomState(23)
    for A, T, U in ((33, 1700, 1500), (300, 120, 40), (300, 2300, 1100), (1000, 50, 7)):
        y, seq = _case(rs, A, T, U)
        err = _check_f64(cf, octc, y, seq, 0, (A, T, U))
        y32 = np.asfortranarray(y.astype(np.float32))
        with np.errstate(all="ignore"):
            c_ref, g_ref, s_ref = octc.ctc_loss(np.asfortranarray(y32.astype(np.float64)), seq)
            cost, grads, skip = cf.ctc_loss_batch([y32], [seq])
        assert not skip[0] and abs(cost[0] - c_ref) <= 1e-11 * abs(c_ref)
        assert np.abs(grads[0].astype(np.float64) - g_ref).max() < 2e-7
        print("A=%d T=%d U=%d: float64 gradient error %.1e" % (A, T, U, err))


def test_wide_alphabet_through_the_network(mods):
    """NNet.costAndGrad with 300 output symbols (brnn_engine.hip no longer bounds the alphabet): softmax, CTC and
    the output layer's gradients against the float64 oracle"""
    cf, octc, torch = mods
    from nnets import brnnet
    from oracle import brnn as obrnn
    D, A, H, NL, TL, T, U = 12, 300, 32, 3, 2, 40, 9
    rs = np.random.RandomState(4)
    data = rs.randn(D, T)
    labels = rs.randint(1, A, size=U).astype(np.int32)
    np.random.seed(9)
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL)
    net.initParams()
    np.random.seed(9)
    params = obrnn.init_params(D, A, H, NL, TL)
    cost, grad, skip = net.costAndGrad(data, labels)
    c_ref, g_ref, s_ref, _ = obrnn.cost_and_grad(params, data, labels, TL, max_act=20.0)
    assert not skip and not s_ref
    assert abs(cost - c_ref) <= 1e-4 * abs(c_ref), (cost, c_ref)
    for (dw, db), gw, gb in zip(grad[:NL + 1], g_ref["W"], g_ref["b"]):
        assert np.linalg.norm(dw.copy_to_host() - gw) <= 1e-4 * np.linalg.norm(gw) + 1e-7
        assert np.linalg.norm(db.copy_to_host().ravel() - gb.ravel()) <= 1e-4 * np.linalg.norm(gb) + 1e-7


def test_long_label_row_through_the_network_and_the_trainer_check(mods):
    """NNet.costAndGrad on utterances whose label row has 2201 lattice states (rounds 1-4: SCTC_ERR_ARG, the trainer
    skipped them): one that fits the workspace's share of 2048 states per frame (T = 1300) and, round 6, one that does
    NOT (T = 2000 = maxBatch: round 5 returned SCTC_ERR_WORKSPACE and the trainer skipped it) -- the model grows its CTC
    scratch for that minibatch (sctc_brnn_ctc_workspace_bytes / sctc_brnn_set_ctc_workspace), like the reference, which
    allocates (2U+1) x T per call (ctc_fast.pyx:22-32).  Cost and gradients against the float64 oracle; a minibatch of a
    long and a short row; the C entries' argument checks"""
    cf, octc, torch = mods
    import ctypes
    from nnets import brnnet
    from oracle import brnn as obrnn
    import sgd
    import _sctc
    D, A, H, NL, TL, U, maxBatch = 8, 20, 32, 2, 1, 1100, 2000
    assert sgd.lattice_fits(1300, U, maxBatch) and sgd.lattice_fits(8000, 800, 8000)
    assert not sgd.lattice_fits(2000, 1100, maxBatch) and sgd.lattice_fits(2000, 1023, maxBatch)
    rs = np.random.RandomState(8)
    np.random.seed(3)
    net = brnnet.NNet(D, A, H, NL, maxBatch, temporalLayer=TL)
    net.initParams()
    np.random.seed(3)
    params = obrnn.init_params(D, A, H, NL, TL)
    for T in (1300, 2000):
        data = rs.randn(D, T)
        labels = rs.randint(1, A, size=U).astype(np.int32)
        cost, grad, skip = net.costAndGrad(data, labels)
        with np.errstate(all="ignore"):
            c_ref, g_ref, s_ref, _ = obrnn.cost_and_grad(params, data, labels, TL, max_act=20.0)
        assert not skip and not s_ref
        assert abs(cost - c_ref) <= 1e-4 * abs(c_ref), (T, cost, c_ref)
        for (dw, db), gw in zip(grad[:NL + 1], g_ref["W"]):
            assert np.linalg.norm(dw.copy_to_host() - gw) <= 2e-4 * np.linalg.norm(gw) + 1e-7
        assert (getattr(net, "_ctc_ws", None) is not None) == (T == 2000)     # grown only when the share is too small
    # a minibatch: the long row next to a short one (the generic path's scratch rows take the widest row of the batch,
    # ADVICE r05), against the two single-utterance results
    netb = brnnet.NNet(D, A, H, NL, maxBatch, temporalLayer=TL, maxUtts=2)
    netb.setParams([[w.copy_to_host(), b.copy_to_host()] for w, b in net.stack])
    datas = [rs.randn(D, 1200), rs.randn(D, 800)]
    labs = [rs.randint(1, A, size=U).astype(np.int32), rs.randint(1, A, size=30).astype(np.int32)]
    costs, _, skips = netb.costAndGradBatch(datas, labs)
    with np.errstate(all="ignore"):
        cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    assert not skips.any() and not sr.any()
    np.testing.assert_allclose(costs, cr, rtol=1e-4)
    for (dw, db), gw in zip(netb.grad[:NL + 1], gr["W"]):
        assert np.linalg.norm(dw.copy_to_host() - gw) <= 2e-4 * np.linalg.norm(gw) + 1e-7
    # the C entries: what a minibatch needs against what the handle offers; argument errors
    L = _sctc.lib()
    mb, keep = netb._minibatch(netb._stage(datas), [1200, 800], labs)
    need, have = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.sctc_brnn_ctc_workspace_bytes(netb._h, ctypes.byref(mb), ctypes.byref(need), ctypes.byref(have)) == 0
    assert 0 < need.value <= have.value
    assert L.sctc_brnn_set_ctc_workspace(netb._h, ctypes.c_void_p(256), 0) == -1
    assert L.sctc_brnn_set_ctc_workspace(netb._h, None, 0) == 0          # back to the built-in share
    assert L.sctc_brnn_ctc_workspace_bytes(netb._h, ctypes.byref(mb), ctypes.byref(need), ctypes.byref(have)) == 0
    netf = brnnet.NNet(D, A, H, NL, 100, train=False, temporalLayer=TL)
    netf.setParams([[w.copy_to_host(), b.copy_to_host()] for w, b in net.stack])
    assert L.sctc_brnn_set_ctc_workspace(netf._h, None, 0) == -1     # a forward-only model has no CTC


def test_32bit_rows_where_the_overlap_is_denormal(mods):
    """The cfg-5 utterance shape (T = 8000, U = 800) on flat random probabilities is where the reference's own per-frame
    scaling runs out of float64: around t = U and t = T - U the overlap sum_s alpha_t[s] beta_t[s] of the two normalised rows
    is 1e-317 (a denormal with seven significant bits) or underflows to 0 (the reference then returns grad = y for the
    frame).  What the reference computes there is rounding noise of ITS operation order; a row store that rounds one factor
    to 22 mantissa bits (the 32-bit rows of the two fused kernels) reproduces it to 2e-6, everything else to 2e-7 -- pinned
    here frame by frame against a NumPy restatement of the lattices; float64 rows (SCTC_CTC_STORE=64) and the lattice + grad
    kernels reproduce the noise too."""
    cf, octc, _ = mods
    from tests import test_ctc_store_model as model
    T, U, A = 8000, 800, 33
    y, seq = model.inputs(T, U, A, 12)          # (seed 12: the model's worst of 20 seeds, 8e-7)
    al, be, lab = model.both(y, seq)
    overlap = (al * be).sum(axis=1)
    assert overlap.min() == 0.0 and (overlap < 1e-300).sum() > 20        # the shape does what the docstring says
    with np.errstate(all="ignore"):
        c_ref, g_ref, s_ref = octc.ctc_loss(y, seq)
    y32 = np.asfortranarray(y.astype(np.float32))                        # (exact: the model's inputs are float32 values)
    assert not s_ref and (y32.astype(np.float64) == y).all()
    sound = overlap > 1e-290
    for which, bound_noise in (("widemin1", 5e-6), ("wide64", 2e-7), ("lattice", 2e-7)):
        with path(which), np.errstate(all="ignore"):
            cost, grads, skip = cf.ctc_loss_batch([y32], [seq])
        assert not skip[0] and abs(cost[0] - c_ref) <= 1e-11 * abs(c_ref)
        err = np.abs(grads[0].astype(np.float64) - g_ref).max(axis=0)     # per frame
        assert err[sound].max() < 2e-7, (which, err[sound].max())
        assert err[~sound].max() < bound_noise, (which, err[~sound].max())
        print("%s: worst |grad - oracle| %.1e where the overlap is a normal number (%d frames), %.1e where it is not (%d)"
              % (which, err[sound].max(), sound.sum(), err[~sound].max(), (~sound).sum()))


def test_cfg5_rows_at_18_utterances_through_the_network(mods):
    """BASELINE configs[4]'s utterance shape (T = 8000, U = 800: 1601 lattice states, 33 symbols) at the smallest
    minibatch the dispatch gives to the wide fused kernel (18), through NNet.costAndGradBatch on a small network:
    costs and gradients against the float64 oracle and against the lattice + grad kernels (SCTC_CTC_WIDE=0)"""
    cf, octc, torch = mods
    from nnets import brnnet
    from oracle import brnn as obrnn
    D, A, H, NL, TL, B, T, U = 6, 33, 16, 2, 1, 18, 8000, 800
    rs = np.random.RandomState(21)
    datas = [rs.randn(D, T) for _ in range(B)]
    labs = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
    np.random.seed(5)
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B)
    net.initParams()
    np.random.seed(5)
    params = obrnn.init_params(D, A, H, NL, TL)
    with np.errstate(all="ignore"):
        cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    res = {}
    for which in ("fused", "lattice"):
        with path(which):
            costs, _, skips = net.costAndGradBatch(datas, labs)
        assert not skips.any() and not sr.any()
        np.testing.assert_allclose(costs, cr, rtol=1e-4)
        for (dw, db), gw in zip(net.grad[:NL + 1], gr["W"]):
            assert np.linalg.norm(dw.copy_to_host() - gw) <= 3e-4 * np.linalg.norm(gw) + 1e-7, which
        res[which] = (costs.copy(), net.grad.flat.clone())
    d = float((res["fused"][1] - res["lattice"][1]).double().norm() / res["lattice"][1].double().norm())
    assert 0 < d < 1e-5, d


def test_wide_rows_through_the_network(mods):
    """NNet.costAndGradBatch on a minibatch of 25 utterances with label rows of 601..1201 lattice states: the engine's CTC
    call takes the wide fused kernel (18 utterances or more, 24 for rows of up to 1024 states; packed-minibatch row layout, float32 probabilities, 32-bit
    rows) -- costs and every gradient against the float64 oracle, and against the same minibatch on the lattice + grad
    kernels (SCTC_CTC_WIDE=0)"""
    cf, octc, torch = mods
    from nnets import brnnet
    from oracle import brnn as obrnn
    D, A, H, NL, TL, B = 8, 20, 32, 2, 1, 25
    rs = np.random.RandomState(12)
    Us = [int(rs.randint(300, 601)) for _ in range(B)]
    Ts = [int(u + rs.randint(60, 400)) for u in Us]
    datas = [rs.randn(D, t) for t in Ts]
    labs = [rs.randint(1, A, size=u).astype(np.int32) for u in Us]
    np.random.seed(3)
    net = brnnet.NNet(D, A, H, NL, max(Ts), temporalLayer=TL, maxUtts=B)
    net.initParams()
    np.random.seed(3)
    params = obrnn.init_params(D, A, H, NL, TL)
    with np.errstate(all="ignore"):
        cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    res = {}
    for which in ("fused", "lattice"):           # "fused" = default switches: the wide kernel at 25 utterances
        with path(which):
            costs, _, skips = net.costAndGradBatch(datas, labs)
        assert not skips.any() and not sr.any()
        np.testing.assert_allclose(costs, cr, rtol=1e-4)
        for (dw, db), gw in zip(net.grad[:NL + 1], gr["W"]):
            assert np.linalg.norm(dw.copy_to_host() - gw) <= 2e-4 * np.linalg.norm(gw) + 1e-7, which
        res[which] = (costs.copy(), net.grad.flat.clone())
    assert np.abs(res["fused"][0] - res["lattice"][0]).max() <= 1e-9 * np.abs(cr).max()
    d = float((res["fused"][1] - res["lattice"][1]).double().norm() / res["lattice"][1].double().norm())
    assert d < 1e-5, d
    assert d > 0, "both runs took the same kernels?"


@pytest.mark.parametrize("which", ["fused", "fused2w", "wide", "lattice", "generic"])
def test_tiny_cost_is_the_log_of_the_band_sum_itself(mods, which):
    """one frame whose blank + label probabilities sum to 1 - 1e-8: the cost is 1e-8 and every path must return the
    logarithm of that very sum (rounds 1-4 took the logarithm of the applied reciprocal: 2e-8 relative error, found
    by the round-5 fuzz soak, seed 5 case 131); a longer utterance of such frames likewise"""
    cf, octc, _ = mods
    with path(which):
        for T, U in ((1, 1), (1, 20), (2, 1), (9, 2)):
            y = np.zeros((3, T))
            y[0], y[1], y[2] = 0.25, 0.75 - 1e-8, 1e-8
            seq = np.full(U, 1, dtype=np.int32)
            if U == 2:
                seq[1] = 2
                y[2], y[1] = 0.5, 0.25 - 1e-8          # label 2 must be reachable
            y = np.asfortranarray(y)
            with np.errstate(all="ignore"):
                c_ref, g_ref, s_ref = octc.ctc_loss(y, seq)
                cost, grad, skip = cf.ctc_loss(y, seq)
            assert bool(skip) == bool(s_ref)
            if not s_ref and np.isfinite(c_ref):
                assert abs(cost - c_ref) <= 1e-10 * abs(c_ref) + 1e-300, (which, T, U, cost, c_ref)
                assert np.abs(grad - g_ref).max() < 1e-9


# ---------------------------------------------------------------- bit-identical outputs, every kernel instantiation

BITS_RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "ctc_bits_parent.txt")
# label rows (U, T) by states per lane and waves: 61, 201, 401, 801 and 1201 lattice states
_ROWS = {2: (30, 77), 4: (100, 230), 8: (200, 300), 16: (400, 520), 32: (600, 690)}
_BITS_PATHS = [  # (path.ENV name, rows, alphabets, dtypes)
    ("fused", (2, 4, 8), (33, 100, 200), "fd"), ("fused64", (2, 4, 8), (33, 100, 200), "f"),
    ("fused2w", (2, 4, 8), (33, 100, 200), "fd"), ("fused2wd", (2, 4), (33,), "f"),
    ("wide", (8, 16, 32), (33, 100, 200), "fd"), ("wide8", (8,), (33, 100, 200), "fd"), ("wide64", (8, 32), (33, 100, 200), "f"),
    ("lattice", (2, 4, 8, 16, 32), (33, 100, 200), "fd"), ("lattice1", (8, 16, 32), (33, 100, 200), "fd"),
    ("lattice4", (32,), (33, 100, 200), "fd"), ("lattice8", (8,), (33, 100, 200), "fd"), ("generic", (2,), (33,), "fd"),
]


def bits_cases():
    """(name, path, A, T, U, blank, dtype, kind): per path every row width, alphabet width and dtype that selects another
    kernel instantiation (tests/test_ctc_plan_cpu.py checks which), the blank id alternating between 0 and A - 1; then
    per path an input that skips (a zero column in phase 1), an empty band (T < U) and T = 1"""
    out = []
    for which, rows, alphabets, dts in _BITS_PATHS:
        shapes = [(A, _ROWS[r][1], _ROWS[r][0], "plain") for r in rows for A in alphabets]
        shapes += [(33, 40, 5, "skip"), (33, 5, 9, "empty"), (33, 1, 1, "plain")]
        for i, (A, T, U, kind) in enumerate(shapes):
            for dt in (dts if kind == "plain" and T > 1 else dts[:1]):
                blank = 0 if (i + (dt == "d")) % 2 == 0 else A - 1
                name = "%s:A%d:T%d:U%d:b%d:%s:%s" % (which, A, T, U, blank, "f64" if dt == "d" else "f32", kind)
                out.append((name, which, A, T, U, blank, np.float64 if dt == "d" else np.float32, kind))
    return out


def bits_line(cf, case):
    """Inputs that depend on no libm: multiples of 2^-16 below 1/16, exact in float32 and float64 (the CTC kernels do
    not need normalised columns); labels uniform over the symbols that are not the blank."""
    name, which, A, T, U, blank, dt, kind = case
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    y = rs.randint(1, 4096, (A, T)) / 65536.0
    seq = rs.randint(0, A - 1, size=U)
    seq = (seq + (seq >= blank)).astype(np.int32)
    if kind == "skip":
        y[:, (3 * T) // 4] = 0.0
    with path(which), np.errstate(all="ignore"):
        cost, grads, skip = cf.ctc_loss_batch([np.asfortranarray(y.astype(dt))], [seq], blank)
    h = hashlib.sha256(np.float64(cost[0]).tobytes() + np.ascontiguousarray(grads[0].T).tobytes() + bytes([int(skip[0])]))
    return "%s %d %s %s" % (name, int(skip[0]), float(cost[0]).hex(), h.hexdigest())


def bits_recorded():
    return [l for l in open(BITS_RECORDED).read().splitlines() if l and not l.startswith("#")]


def test_outputs_are_bit_identical_to_the_recorded_parent(mods):
    """Every CTC kernel instantiation's cost, gradient and skip flag, bit for bit (a SHA-256 per case), against
    tests/data/ctc_bits_parent.txt: the kernels sum in fixed trees and fixed list orders, so a change that only moves
    code must reproduce every bit, and one that changes a rounding shows up here and not only where a tolerance runs out.

    The file was recorded on an MI355X from a build of commit d852786 (the parent of the change that introduced
    csrc/ctc_dev.h), through this very code: the Python layer did not change, so that commit's library was loaded into this
    tree with SCTC_LIB_PATH and `python -m tests.test_gpu_ctc_paths` run twice, in two processes; the two outputs were
    equal line for line (a case whose two recordings differ would be left out of the file: the test runs the recorded
    lines only, and tests/test_ctc_plan_cpu.py checks that they still reach every instantiation).  To repeat it: check
    that commit out, build it, and run the same command with SCTC_LIB_PATH pointing at its libsctc_hip.so.  After a
    change that is MEANT to change bits, record again from the new build and say so."""
    cf, _, _ = mods
    cases = {c[0]: c for c in bits_cases()}
    recorded = bits_recorded()
    assert len(recorded) > 150 and all(l.split()[0] in cases for l in recorded)
    differ = []
    for want in recorded:
        got = bits_line(cf, cases[want.split()[0]])
        if got != want:
            differ.append((got, want))
    assert not differ, "%d of %d cases differ, the first: got %r, recorded %r" % (len(differ), len(recorded), differ[0][0], differ[0][1])


if __name__ == "__main__":      # the recording (see the test's docstring)
    import sys
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "stanford-ctc_amd")]
    import ctc_fast
    for _case in bits_cases():
        print(bits_line(ctc_fast, _case), flush=True)
