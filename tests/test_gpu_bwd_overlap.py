"""The overlap order of the backward pass (SCTC_BWD_OVERLAP, csrc/bwd_overlap_plan.h): the weight gradients above the
temporal layer run beside the BPTT grid -- the default grid with the larger LDS claim (1) or the half grid (2) -- on a
stream and a delta-buffer route of their own (they share the step's split-K workspace, which nothing else uses
meanwhile).  Same kernels, tiles and splits as the serial order (0), and the half grid keeps the K split and the order of every addition: costs, skips and EVERY gradient (weights, biases, both
recurrent matrices) are bit for bit those of the serial order, over plain and accumulating steps, equal and ragged lengths,
17 and 32 utterances, with the L2 term.  Where the overlap does not apply (one H x H gradient above the temporal layer,
a forced recurrent variant, the synchronising timers) the pass takes the serial order and says so."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, A, NL, TMAX = 40, 9, 5, 24


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import _sctc
    from nnets import brnnet
    from oracle import brnn as obrnn
    return brnnet, obrnn, _sctc


_PARAMS = {}


def _params(obrnn, H, TL):
    if (H, TL) not in _PARAMS:
        _PARAMS[H, TL] = obrnn.init_params(D, A, H, NL, TL, rng=np.random.RandomState(1000 + H + TL))
    return _PARAMS[H, TL]


def _net(brnnet, params, H, TL, B):
    net = brnnet.NNet(D, A, H, NL, TMAX, temporalLayer=TL, maxUtts=B, reg=0.01)
    net.maxAct = 20.0
    net.setParams([[w, b] for w, b in zip(params["W"], params["b"])] + [[params["Wf"], None], [params["Wb"], None]])
    return net


def _batch(rs, B, ragged):
    Ts = [int(t) for t in rs.randint(2, TMAX + 1, size=B)] if ragged else [TMAX] * B
    Ts[0] = TMAX
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 4)).astype(np.int32) for T in Ts]
    return datas, labs


def _snapshot(net, res):
    costs, _, skips = res
    grads = []
    for i in range(NL + 1):
        grads += [net.grad[i][0].copy_to_host().copy(), net.grad[i][1].copy_to_host().copy()]
    grads += [net.grad[NL + 1][0].copy_to_host().copy(), net.grad[NL + 2][0].copy_to_host().copy()]
    return costs.copy(), skips.copy(), grads


def _steps(net, batches):
    """two plain steps, then one that accumulates into the second's gradients: a snapshot behind each"""
    out = []
    for k, (datas, labs) in enumerate(batches):
        out.append(_snapshot(net, net.costAndGradBatch(datas, labs, accumulate=(k == 2))))
    return out


def _assert_same(got, want):
    assert len(got) == len(want)
    for (c1, s1, g1), (c0, s0, g0) in zip(got, want):
        np.testing.assert_array_equal(c1, c0)
        np.testing.assert_array_equal(s1, s0)
        assert np.isfinite(c0[~s0.astype(bool)]).all()
        assert len(g1) == len(g0) == 2 * (NL + 1) + 2
        for a, b in zip(g1, g0):
            assert np.isfinite(b).all()
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [17, 32])
@pytest.mark.parametrize("H", [1824, 2048])
def test_overlap_orders_are_bit_identical_to_the_serial_order(mods, monkeypatch, H, B, ragged):
    brnnet, obrnn, _ = mods
    TL = 3
    rs = np.random.RandomState(11 * H + B + int(ragged))
    params = _params(obrnn, H, TL)
    batches = [_batch(rs, B, ragged) for _ in range(3)]
    res = {}
    for mode in (0, 1, 2):
        monkeypatch.setenv("SCTC_BWD_OVERLAP", str(mode))
        net = _net(brnnet, params, H, TL, B)
        res[mode] = _steps(net, batches)
        assert net.recurrentPath()[:2] == (1, 1)
        assert net.bwdOverlapMode() == mode
        del net
    _assert_same(res[1], res[0])
    _assert_same(res[2], res[0])


def test_one_square_gradient_above_the_temporal_layer_takes_the_serial_order(mods, monkeypatch):
    brnnet, obrnn, _ = mods
    H, B, TL = 1824, 32, 4
    rs = np.random.RandomState(5)
    params = _params(obrnn, H, TL)
    batches = [_batch(rs, B, True) for _ in range(3)]
    res = {}
    for mode in (0, 2):
        monkeypatch.setenv("SCTC_BWD_OVERLAP", str(mode))
        net = _net(brnnet, params, H, TL, B)
        res[mode] = _steps(net, batches)
        assert net.bwdOverlapMode() == 0
        del net
    _assert_same(res[2], res[0])


def test_forced_fallback_recurrence_takes_the_serial_order(mods, monkeypatch):
    brnnet, obrnn, _ = mods
    H, B, TL = 1824, 17, 3
    rs = np.random.RandomState(6)
    params = _params(obrnn, H, TL)
    batches = [_batch(rs, B, True) for _ in range(3)]
    monkeypatch.setenv("SCTC_REC_VARIANT", "3")
    res = {}
    for mode in (0, 1, 2):
        monkeypatch.setenv("SCTC_BWD_OVERLAP", str(mode))
        net = _net(brnnet, params, H, TL, B)
        res[mode] = _steps(net, batches)
        assert net.recurrentPath()[:2] == (3, 3)
        assert net.bwdOverlapMode() == 0
        del net
    _assert_same(res[1], res[0])
    _assert_same(res[2], res[0])


@pytest.mark.parametrize("mode", [1, 2])
def test_phase_timers_under_the_overlap_order(mods, monkeypatch, mode):
    brnnet, obrnn, _sctc = mods
    H, B, TL = 1824, 32, 3
    rs = np.random.RandomState(7)
    params = _params(obrnn, H, TL)
    datas, labs = _batch(rs, B, False)
    monkeypatch.setenv("SCTC_BWD_OVERLAP", str(mode))
    net = _net(brnnet, params, H, TL, B)
    L = _sctc.lib()
    arr = (ctypes.c_float * 6)()
    want = _snapshot(net, net.costAndGradBatch(datas, labs))
    assert net.bwdOverlapMode() == mode
    for profiling, ran in ((1, 0), (2, mode)):      # the synchronising timers take the serial order
        L.sctc_brnn_set_profiling(net._h, profiling)
        got = _snapshot(net, net.costAndGradBatch(datas, labs))
        assert L.sctc_brnn_phase_ms(net._h, arr) == 0
        L.sctc_brnn_set_profiling(net._h, 0)
        ms = np.array(list(arr), dtype=np.float64)
        assert net.bwdOverlapMode() == ran
        assert np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0
        _assert_same([got], [want])
