"""GPU parity of the BRNN step (nnets.brnnet.NNet through the C ABI) against the CPU
oracle and the golden vectors produced by the reference's rnnetcpu.py -- the re-creation
of ctc_fast/debug-utils/checkgrads.py:20-40 (GPU fp32 vs CPU fp64, same seed, same init).

Tolerances (fp32 device arithmetic vs fp64 oracle): cost 1e-4 relative (north_star),
gradients 1e-4 relative Frobenius norm per tensor at these sizes (observed ~3e-7; SURVEY 8(c)
allows 1e-3).  The full-size configurations (thousands of dependent fp32 steps) have their own
stated tolerance in tests/test_gpu_fullsize.py.
"""
import io
import pickle

import os

import numpy as np
import pytest

from tests.helpers import load_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import _sctc
    from nnets import brnnet
    from oracle import brnn as obrnn
    return _sctc, brnnet, obrnn, torch


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def gemm_mode(request, monkeypatch):
    """every test of this file runs twice: with the fp32 matrix-core instruction (the reference's
    arithmetic, the benchmarked path) and with the fp32-accurate three-term bfloat16 split
    (NNet(..., gemm="bf16x3")) -- same oracle, same tolerances (VERDICT r02 #3c: in the suite, not
    behind an environment variable of a separate run)"""
    monkeypatch.setenv("SCTC_GEMM", request.param)
    return request.param


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-30)


def host_stack(params):
    st = [[w, b] for w, b in zip(params["W"], params["b"])]
    if params["Wf"] is not None:
        st += [[params["Wf"], None], [params["Wb"], None]]
    return st


def make_net(brnnet, dims, params, maxUtts=1, reg=0.0, max_act=20.0, train=True, maxBatch=None, gemm=None):
    D, A, H, NL, TL, T = dims
    net = brnnet.NNet(D, A, H, NL, maxBatch or T, train=train, temporalLayer=TL, reg=reg,
                      maxUtts=maxUtts, gemm=gemm)
    net.maxAct = max_act
    net.setParams(host_stack(params))
    return net


def check_grads(net, grads, NL, tol=1e-4):
    worst = 0.0
    for i in range(NL + 1):
        dw, db = net.grad[i]
        worst = max(worst, rel(dw.copy_to_host(), grads["W"][i]))
        worst = max(worst, rel(db.copy_to_host().reshape(-1), np.asarray(grads["b"][i]).reshape(-1)))
    if grads["Wf"] is not None:
        worst = max(worst, rel(net.grad[NL + 1][0].copy_to_host(), grads["Wf"]))
        worst = max(worst, rel(net.grad[NL + 2][0].copy_to_host(), grads["Wb"]))
    assert worst < tol, worst
    return worst


def test_gemm_all_layouts(mods):
    """sctc_gemm_f32 (== cm.dot) in the four operand layouts, ragged sizes, vs float64 NumPy"""
    _sctc, _, _, torch = mods
    L = _sctc.lib()
    rs = np.random.RandomState(0)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    for (M, N, K) in ((200, 96, 64), (130, 260, 1824), (1000, 1824, 512), (64, 1824, 3000),
                      (1824, 512, 777), (32, 32, 4)):
        for akc in (1, 0):
            for bkc in (1, 0):
                if (akc and K % 4) or (not akc and M % 4) or (bkc and K % 4) or (not bkc and N % 4):
                    continue
                A = rs.randn(M, K).astype(np.float32)
                Bm = rs.randn(K, N).astype(np.float32)
                bias = rs.randn(N).astype(np.float32)
                a_dev = torch.from_numpy(np.ascontiguousarray(A if akc else A.T)).cuda()
                b_dev = torch.from_numpy(np.ascontiguousarray(Bm.T if bkc else Bm)).cuda()
                c_dev = torch.full((M, N), 7.0, dtype=torch.float32, device="cuda")
                bias_dev = torch.from_numpy(bias).cuda()
                rc = L.sctc_gemm_f32(a_dev.data_ptr(), a_dev.shape[1], akc, b_dev.data_ptr(),
                                     b_dev.shape[1], bkc, c_dev.data_ptr(), N, M, N, K,
                                     bias_dev.data_ptr(), 1, ws.data_ptr(), ws.numel(), None)
                _sctc.check(rc, "gemm")
                torch.cuda.synchronize()
                ref = np.maximum(A.astype(np.float64) @ Bm.astype(np.float64) + bias, 0.0)
                err = np.abs(c_dev.cpu().numpy() - ref).max() / np.abs(ref).max()
                assert err < 2e-6, (M, N, K, akc, bkc, err)


def test_brnn_main_fixture(mods, golden):
    """rnnetcpu.py __main__ (seed 33): COST 12.023458823 and all gradients"""
    _, brnnet, obrnn, _ = mods
    params, grads, dims, data, labels, cost = load_net(golden("brnn_main.npz"))
    net = make_net(brnnet, dims, params)
    c, g, skip = net.costAndGrad(data, labels)
    assert not skip
    assert c == pytest.approx(cost, rel=1e-4)
    assert c == pytest.approx(12.023458823, rel=1e-4)
    check_grads(net, grads, dims[3])


def test_brnn_init_matches_reference_seed(mods, golden):
    """same seed -> same init as the reference (checkgrads.py:20-28)"""
    _, brnnet, _, _ = mods
    params, _, dims, data, labels, cost = load_net(golden("brnn_main.npz"))
    D, A, H, NL, TL, T = dims
    np.random.seed(33)
    np.random.randn(D, T)
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL)
    net.initParams()
    for (w, b), ref in zip(net.stack[:NL + 1], params["W"]):
        np.testing.assert_allclose(w.copy_to_host(), ref.astype(np.float32), rtol=0, atol=0)
    np.testing.assert_array_equal(net.stack[NL + 1][0].copy_to_host(), params["Wf"].astype(np.float32))
    np.testing.assert_array_equal(net.stack[NL + 2][0].copy_to_host(), params["Wb"].astype(np.float32))
    assert net.stack[NL + 1][1].shape == (1, 1) and net.stack[NL + 1][1] is net.stack[NL + 2][1]
    assert net.paramCount() == sum(int(np.prod(w.shape)) + int(np.prod(b.shape)) for w, b in net.stack)
    c, _, _ = net.costAndGrad(data, labels)
    assert c == pytest.approx(cost, rel=1e-4)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
def test_brnn_scaled_configs(mods, golden, name):
    _, brnnet, _, _ = mods
    params, grads, dims, data, labels, cost = load_net(golden("brnn_cfg.npz"), name + "_")
    net = make_net(brnnet, dims, params)
    c, g, skip = net.costAndGrad(data, labels)
    assert not skip
    assert c == pytest.approx(cost, rel=1e-4)
    check_grads(net, grads, dims[3])


def test_brnn_ceiling_reg_and_masks(mods):
    """clip at maxAct=20, the strict (0,20) mask and L2 reg: only brnnet.py has them"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(5)
    D, A, H, NL, TL, T = 24, 9, 40, 4, 2, 37
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    params["Wf"] *= 1.5
    params["b"][TL - 1] += 4.0
    data = 3.0 * rs.randn(D, T)
    labels = rs.randint(1, A, size=6).astype(np.int32)
    reg = 0.01
    c_ref, g_ref, s_ref, _ = obrnn.cost_and_grad(params, data, labels, TL, 20.0, reg)
    _, cache = obrnn.forward(params, data, TL, 20.0)
    assert (cache["hF"] >= 20.0).any() and (cache["hB"] >= 20.0).any()
    net = make_net(brnnet, (D, A, H, NL, TL, T), params, reg=reg)
    c, g, skip = net.costAndGrad(data, labels)
    assert not skip and not s_ref
    assert c == pytest.approx(c_ref, rel=1e-4)
    assert net.regcost > 0
    check_grads(net, g_ref, NL)


def test_brnn_no_temporal_layer_and_tl_validity(mods):
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(6)
    D, A, H, NL, T = 17, 11, 33, 2, 25
    for TL in (-1, 0, 2, 5):                     # all invalid -> plain DNN (brnnet.py:27-30)
        net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL)
        assert net.temporalLayer == -1
    params = obrnn.init_params(D, A, H, NL, -1, rng=rs)
    data = rs.randn(D, T)
    labels = rs.randint(1, A, size=4).astype(np.int32)
    c_ref, g_ref, _, _ = obrnn.cost_and_grad(params, data, labels, -1)
    net = make_net(brnnet, (D, A, H, NL, -1, T), params)
    assert len(net.stack) == NL + 1
    c, g, skip = net.costAndGrad(data, labels)
    assert c == pytest.approx(c_ref, rel=1e-4)
    check_grads(net, g_ref, NL)


def test_brnn_minibatch_ragged_sum_of_gradients(mods):
    """B ragged utterances in one call == sum of the oracle's per-utterance gradients;
    a skipped (infeasible) utterance contributes nothing"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(7)
    D, A, H, NL, TL = 21, 33, 64, 3, 2
    Ts = [40, 17, 33, 40, 9, 25, 1, 12]
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 6)).astype(np.int32) for T in Ts]
    labs[4] = np.array([3, 3, 3, 3, 3, 3], dtype=np.int32)      # T=9 < 11 needed -> skip
    costs_ref, g_ref, skips_ref, n_valid = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    assert skips_ref[4] and n_valid == len(Ts) - 1
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=len(Ts))
    costs, g, skips = net.costAndGradBatch(datas, labs)
    np.testing.assert_array_equal(skips, skips_ref)
    ok = ~skips_ref
    np.testing.assert_allclose(costs[ok], costs_ref[ok], rtol=1e-4)
    check_grads(net, g_ref, NL)
    # B=1 through the batch entry point is bit-identical to the single-utterance path
    c1, _, _ = net.costAndGradBatch([datas[0]], [labs[0]])
    g_batch = net.grad[0][0].copy_to_host().copy()
    c2, _, _ = net.costAndGrad(datas[0], labs[0])
    assert c1[0] == c2
    np.testing.assert_array_equal(g_batch, net.grad[0][0].copy_to_host())
    # run-to-run reproducibility of the minibatch gradient
    net.costAndGradBatch(datas, labs)
    ga = net.grad[1][0].copy_to_host().copy()
    net.costAndGradBatch(datas, labs)
    np.testing.assert_array_equal(ga, net.grad[1][0].copy_to_host())


def test_brnn_skip_returns_stale_grads(mods):
    """brnnet.py:185-186: on skip the previous gradients are returned untouched"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(8)
    D, A, H, NL, TL, T = 10, 5, 32, 2, 1, 12
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    net = make_net(brnnet, (D, A, H, NL, TL, T), params)
    data = rs.randn(D, T)
    c, g, skip = net.costAndGrad(data, np.array([1, 2], dtype=np.int32))
    assert not skip
    before = net.grad[0][0].copy_to_host().copy()
    c2, g2, skip2 = net.costAndGrad(data[:, :5], np.array([2, 2, 2, 2], dtype=np.int32))
    assert skip2
    np.testing.assert_array_equal(before, net.grad[0][0].copy_to_host())


def test_brnn_forward_only_and_checkpoint(mods):
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(9)
    D, A, H, NL, TL, T = 15, 12, 48, 3, 2, 30
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    data = rs.randn(D, T).astype(np.float32)
    net = make_net(brnnet, (D, A, H, NL, TL, T), params)
    buf = io.BytesIO()
    net.toFile(buf)
    buf.seek(0)
    stack = pickle.load(buf)                      # reference format: list of [w, b] float32
    assert len(stack) == NL + 3 and stack[0][0].dtype == np.float32
    assert stack[0][0].shape == (H, D) and stack[0][1].shape == (H, 1)
    assert stack[-1][0].shape == (H, H) and stack[-1][1].shape == (1, 1)
    buf.seek(0)
    net2 = brnnet.NNet(D, A, H, NL, T, train=False, temporalLayer=TL)
    net2.fromFile(buf)
    probs = net2.costAndGrad(data)                # brnnet.py:171-173
    assert probs.shape == (A, T) and probs.dtype == np.float32
    logits, _ = obrnn.forward(params, data.astype(np.float64), TL, 20.0)
    ref = obrnn.softmax_cols(logits)
    np.testing.assert_allclose(probs, ref, rtol=2e-4, atol=1e-6)
    with pytest.raises(AssertionError):
        net2.costAndGrad(np.zeros((D, T + 1), dtype=np.float32))   # "Batch size exceeds max batch"


def test_brnn_update_params(mods):
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(10)
    D, A, H, NL, TL, T = 8, 5, 32, 2, 1, 6
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    net = make_net(brnnet, (D, A, H, NL, TL, T), params)
    net.costAndGrad(rs.randn(D, T), np.array([1], dtype=np.int32))
    w0 = net.stack[0][0].copy_to_host().copy()
    g0 = net.grad[0][0].copy_to_host().copy()
    net.updateParams(-0.5, net.grad)              # flat fast path
    np.testing.assert_allclose(net.stack[0][0].copy_to_host(), w0 - 0.5 * g0, rtol=1e-6, atol=1e-7)
    vel = net.zerosLikeStack()
    vel[0][0].add_mult(net.grad[0][0], alpha=2.0)
    vel[0][0].mult(0.25)
    np.testing.assert_allclose(vel[0][0].copy_to_host(), 0.5 * g0, rtol=1e-6, atol=1e-7)
    n = net.grad[0][0].euclid_norm()
    assert n == pytest.approx(np.linalg.norm(g0.astype(np.float64)), rel=1e-6)


def test_brnn_full_size_cfg3_vs_oracle(mods):
    """the headline configuration itself (T=1000, 5x1824, A=33, U=100): two utterances through
    the batched GPU path against the float64 oracle, plus the size-independent properties:
    an utterance's cost does not depend on what else is in the minibatch (to fp32 summation order), and the
    minibatch gradient is the sum of the single-utterance gradients"""
    _, brnnet, obrnn, torch = mods
    D, A, H, NL, TL, T, U = 483, 33, 1824, 5, 3, 1000, 100
    rs = np.random.RandomState(0)
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T).astype(np.float32) for _ in range(3)]
    labs = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(3)]
    net = make_net(brnnet, (D, A, H, NL, TL, T), params, maxUtts=3, maxBatch=T)
    costs, _, skips = net.costAndGradBatch(datas, labs)
    g_all = [net.grad[i][0].copy_to_host().astype(np.float64) for i in (0, 2, NL, NL + 1, NL + 2)]
    assert not skips.any()
    with np.errstate(all="ignore"):
        c_ref, g_ref, s_ref, _ = obrnn.cost_and_grad(params, datas[1].astype(np.float64), labs[1], TL, 20.0)
    assert costs[1] == pytest.approx(c_ref, rel=1e-4)                 # north_star tolerance
    assert abs(costs[1] - c_ref) / c_ref < 2e-6                       # what fp32 achieves here
    # batch-composition invariance: rows are independent; only the split-K factor of the
    # GEMMs (chosen from the frame count) changes the fp32 summation order
    c1, _, _ = net.costAndGradBatch([datas[1]], [labs[1]])
    assert c1[0] == pytest.approx(costs[1], rel=1e-6)
    g1 = [net.grad[i][0].copy_to_host().astype(np.float64) for i in (0, 2, NL, NL + 1, NL + 2)]
    for got, want in zip(g1, (g_ref["W"][0], g_ref["W"][2], g_ref["W"][NL], g_ref["Wf"], g_ref["Wb"])):
        assert rel(got, want) < 2e-3
    # additivity over utterances
    acc = [g.copy() for g in g1]
    for j in (0, 2):
        net.costAndGradBatch([datas[j]], [labs[j]])
        for a, i in zip(acc, (0, 2, NL, NL + 1, NL + 2)):
            a += net.grad[i][0].copy_to_host()
    # (different minibatch sizes pick different split-K factors; 1000 recurrent steps amplify the
    # fp32 rounding differences to ~6e-4 on the deepest gradient -- same tolerance as vs the oracle)
    for a, b in zip(acc, g_all):
        assert rel(b, a) < 2e-3


def _all_grads(net, NL):
    return [net.grad[i][0].copy_to_host().astype(np.float64).copy() for i in range(NL + 3)]


@pytest.mark.parametrize("H,NL,TL,B", [(96, 3, 2, 5), (200, 4, 1, 3), (64, 4, 3, 8), (1824, 3, 2, 2), (132, 2, 1, 1)])
def test_sums_around_the_temporal_layer_fused_into_gemms(mods, monkeypatch, gemm_mode, H, NL, TL, B):
    """brnnet.py:153 (hActs = hActsFor + hActsBack) and :233 (deltasOut = deltasFor + deltasBack) are formed
    by the GEMMs that consume them (GemmArgs::A2: two addends summed while the A tile is staged; the sum is
    stored once for its later readers): every cost and gradient is BIT-identical to the step that runs
    add_kernel (SCTC_FUSE_ADD=0) -- temporal layer first, in the middle and last admissible (NL - 1), layer sizes that are and
    are not multiples of the tile shapes, ragged minibatches"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(100 + H)
    D, A = 24, 33
    Ts = [int(t) for t in rs.randint(2, 38, size=B)]
    Ts[0] = 37
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 7)).astype(np.int32) for T in Ts]
    out = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("SCTC_FUSE_ADD", fuse)
        net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B, reg=1e-3)
        costs, _, skips = net.costAndGradBatch(datas, labs)
        out.append((costs.copy(), skips.copy(), _all_grads(net, NL),
                    [net.grad[i][1].copy_to_host().copy() for i in range(NL + 1)]))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    for a, b in zip(out[0][2] + out[0][3], out[1][2] + out[1][3]):
        np.testing.assert_array_equal(a, b)
    if gemm_mode == "f32" and H < 1000:      # and the fused step is the oracle's step
        with np.errstate(all="ignore"):
            _, g_ref, _, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
        monkeypatch.setenv("SCTC_FUSE_ADD", "1")
        net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
        net.costAndGradBatch(datas, labs)
        check_grads(net, g_ref, NL)


def test_recurrent_two_chain_kernel_vs_oracle(mods, monkeypatch):
    """17..32 utterances run the two-chains-per-CU recurrent kernel (recurrent.hip): ragged
    minibatch of 24 at H=512 against the float64 oracle, and against the one-workgroup-per-CU
    kernel (SCTC_REC_VARIANT=1) on the same inputs"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(11)
    D, A, H, NL, TL = 40, 33, 512, 2, 1
    Ts = [int(t) for t in rs.randint(3, 41, size=24)]
    Ts[5] = 40
    Ts[17] = 1
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    with np.errstate(all="ignore"):
        costs_ref, g_ref, skips_ref, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=len(Ts))
    costs, _, skips = net.costAndGradBatch(datas, labs)
    np.testing.assert_array_equal(skips, skips_ref)
    np.testing.assert_allclose(costs[~skips_ref], costs_ref[~skips_ref], rtol=1e-4)
    check_grads(net, g_ref, NL)
    g_q = _all_grads(net, NL)
    monkeypatch.setenv("SCTC_REC_VARIANT", "1")
    net1 = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=len(Ts))
    costs1, _, _ = net1.costAndGradBatch(datas, labs)
    np.testing.assert_allclose(costs, costs1, rtol=1e-6)
    for a, b in zip(g_q, _all_grads(net1, NL)):
        assert rel(a, b) < 1e-5


@pytest.mark.parametrize("H", [1824, 2048, 1024])
def test_recurrent_two_chain_kernel_layer_sizes(mods, monkeypatch, H):
    """the register/LDS weight split (H=1824: 29/29/28/28 chunks per wave, 10 in registers;
    H=2048: 32 per wave, 13 in registers) against the one-workgroup-per-CU kernel"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(H)
    D, A, NL, TL = 32, 33, 2, 1
    Ts = sorted((int(t) for t in rs.randint(8, 25, size=32)), reverse=True)
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=len(Ts))
    costs, _, skips = net.costAndGradBatch(datas, labs)
    assert not skips.any()
    g_q = _all_grads(net, NL)
    monkeypatch.setenv("SCTC_REC_VARIANT", "1")
    net1 = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=len(Ts))
    costs1, _, _ = net1.costAndGradBatch(datas, labs)
    np.testing.assert_allclose(costs, costs1, rtol=1e-5)
    errs = []
    for k, (a, b) in enumerate(zip(g_q, _all_grads(net1, NL))):
        # two kernels = two fp32 summation orders: a unit whose pre-activation sits on the clip /
        # ReLU kink can land on either side, and its delta is then present in one result only.
        # That shows in dW1 alone (zero-mean inputs: a random-walk norm with no coherent part;
        # tests/test_gpu_fullsize.py::test_cfg4_input_layer_gradient_error_decomposed)
        errs.append(rel(a, b))
    assert errs[0] < 3e-3 and max(errs[1:]) < 3e-4, ["%.1e" % e for e in errs]
    # one utterance of the minibatch against the oracle
    with np.errstate(all="ignore"):
        c_ref, _, _, _ = obrnn.cost_and_grad(params, datas[20], labs[20], TL, 20.0)
    assert costs[20] == pytest.approx(c_ref, rel=1e-4)


@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_recurrent_small_batch_kernel_vs_oracle(mods, monkeypatch, B):
    """1..5 utterances run the sentinel-exchange / register-weight recurrent kernel
    (recurrent.hip, brnn_recurrent_s_kernel): ragged minibatch at H=512 against the float64
    oracle and against the flag-based MFMA kernel (SCTC_REC_VARIANT=1)"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(100 + B)
    D, A, H, NL, TL = 40, 33, 512, 2, 1
    Ts = [37, 12, 1, 25, 30, 9, 37, 18][:B]
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    with np.errstate(all="ignore"):
        costs_ref, g_ref, skips_ref, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
    costs, _, skips = net.costAndGradBatch(datas, labs)
    np.testing.assert_array_equal(skips, skips_ref)
    np.testing.assert_allclose(costs[~skips_ref], costs_ref[~skips_ref], rtol=1e-4)
    check_grads(net, g_ref, NL)
    g_s = _all_grads(net, NL)
    # run-to-run reproducibility (fixed summation order, no arrival-order dependence)
    net.costAndGradBatch(datas, labs)
    for a, b in zip(g_s, _all_grads(net, NL)):
        np.testing.assert_array_equal(a, b)
    monkeypatch.setenv("SCTC_REC_VARIANT", "1")
    net1 = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
    costs1, _, _ = net1.costAndGradBatch(datas, labs)
    np.testing.assert_allclose(costs, costs1, rtol=1e-6)
    for a, b in zip(g_s, _all_grads(net1, NL)):
        assert rel(a, b) < 1e-5


@pytest.mark.parametrize("H", [1824, 2048, 1024])
def test_recurrent_small_batch_kernel_layer_sizes(mods, monkeypatch, H):
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(7 * H)
    D, A, NL, TL = 32, 33, 2, 1
    Ts = [40, 33]
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=2)
    costs, _, skips = net.costAndGradBatch(datas, labs)
    assert not skips.any()
    g_s = _all_grads(net, NL)
    monkeypatch.setenv("SCTC_REC_VARIANT", "1")
    net1 = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=2)
    costs1, _, _ = net1.costAndGradBatch(datas, labs)
    np.testing.assert_allclose(costs, costs1, rtol=1e-5)
    for a, b in zip(g_s, _all_grads(net1, NL)):
        assert rel(a, b) < 1e-4
    with np.errstate(all="ignore"):
        c_ref, _, _, _ = obrnn.cost_and_grad(params, datas[1], labs[1], TL, 20.0)
    assert costs[1] == pytest.approx(c_ref, rel=1e-4)


@pytest.mark.parametrize("H,B", [(512, 6), (512, 16), (1824, 9), (2048, 12), (1024, 7), (1824, 16)])
def test_recurrent_mid_batch_kernel(mods, monkeypatch, H, B):
    """6..16 utterances (4..16 since the crossover measurement): since round 5 the flag kernel with ONE chain per
    direction (brnn_recurrent_q_kernel on half its grid).  Ragged minibatch against the one-workgroup-per-CU flag
    kernel (SCTC_REC_VARIANT=1) and, at H=512, the oracle.  (The sentinel-exchange MFMA kernel it replaced,
    brnn_recurrent_m_kernel, agreed bit for bit in round 5; it left the tree after commit 1cbab82.)"""
    variant = "0"
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(31 * H + B)
    D, A, NL, TL = 32, 33, 2, 1
    Ts = [int(t) for t in rs.randint(2, 30, size=B)]
    Ts[0] = 30
    Ts[-1] = 1
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    monkeypatch.setenv("SCTC_REC_VARIANT", variant)
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
    costs, _, skips = net.costAndGradBatch(datas, labs)
    assert net.recurrentPath()[:2] == (1, 1)
    g_m = _all_grads(net, NL)
    net.costAndGradBatch(datas, labs)
    for a, b in zip(g_m, _all_grads(net, NL)):
        np.testing.assert_array_equal(a, b)          # run-to-run reproducible
    if H == 512:
        with np.errstate(all="ignore"):
            costs_ref, g_ref, skips_ref, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
        np.testing.assert_array_equal(skips, skips_ref)
        np.testing.assert_allclose(costs[~skips_ref], costs_ref[~skips_ref], rtol=1e-4)
        check_grads(net, g_ref, NL)
    monkeypatch.setenv("SCTC_REC_VARIANT", "1")
    net1 = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
    costs1, _, _ = net1.costAndGradBatch(datas, labs)
    np.testing.assert_allclose(costs[~skips], costs1[~skips], rtol=1e-5)
    for a, b in zip(g_m, _all_grads(net1, NL)):
        assert rel(a, b) < 1e-4


@pytest.mark.parametrize("H,B", [(64, 40), (512, 48), (512, 70)])
def test_recurrent_large_minibatch(mods, H, B):
    """more than 32 utterances: several utterance tiles per wave in the one-workgroup-per-CU
    recurrent kernel (NTW = 2 / 4), ragged, against the float64 oracle"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(5 * H + B)
    D, A, NL, TL = 24, 33, 2, 1
    Ts = [int(t) for t in rs.randint(1, 22, size=B)]
    Ts[3] = 22
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
    # The reference's init saturates most units at the [0,20] clip; a unit that sits within fp32 rounding of a boundary
    # gets its mask from the summation order of the kernel that happens to run (tests/gpu_fuzz.py: such a difference
    # must disappear under a 1e-5 relative perturbation of the inputs -- a real defect would not).  (512, 48) is such a
    # case for the round-5 dispatch (32 + 16 utterances as two launches): one unit of the forward recurrence, dW1 / dWf
    # 5.8e-4 / 3.2e-4 off at eps = 0, 2e-7 at 1e-5; tools/rec_split_check.py.
    for eps in (0.0, 1e-5, 1e-4):
        dd = [d * (1.0 + eps) for d in datas]
        with np.errstate(all="ignore"):
            costs_ref, g_ref, skips_ref, _ = obrnn.cost_and_grad_batch(params, dd, labs, TL)
        costs, _, skips = net.costAndGradBatch(dd, labs)
        np.testing.assert_array_equal(skips, skips_ref)
        np.testing.assert_allclose(costs[~skips_ref], costs_ref[~skips_ref], rtol=1e-4)
        try:
            check_grads(net, g_ref, NL)
            break
        except AssertionError:
            if eps == 1e-4:
                raise


def test_recurrent_more_than_128_utterances(mods):
    """minibatches beyond one launch's 128 utterances run as consecutive launches of the
    persistent kernels (utterances are independent): 150 ragged utterances against the oracle"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(77)
    D, A, H, NL, TL, B = 16, 12, 64, 2, 1, 150
    Ts = [int(t) for t in rs.randint(1, 15, size=B)]
    Ts[5] = 15
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 6)).astype(np.int32) for T in Ts]
    with np.errstate(all="ignore"):
        costs_ref, g_ref, skips_ref, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
    costs, _, skips = net.costAndGradBatch(datas, labs)
    np.testing.assert_array_equal(skips, skips_ref)
    np.testing.assert_allclose(costs[~skips_ref], costs_ref[~skips_ref], rtol=1e-4)
    check_grads(net, g_ref, NL)


def test_async_entry_matches_sync(mods):
    """sctc_brnn_cost_and_grad_async + sctc_brnn_check (the data-parallel trainer's entry): same
    costs, skip flags and bit-identical gradients as the synchronous call; the gradient-ready
    events cover the flat buffer exactly once in backward order (output layer first)"""
    _, brnnet, obrnn, torch = mods
    rs = np.random.RandomState(21)
    D, A, H, NL, TL = 21, 33, 64, 4, 2
    Ts = [30, 12, 25, 7, 30, 18]
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 6)).astype(np.int32) for T in Ts]
    labs[3] = np.array([4, 4, 4, 4, 4], dtype=np.int32)          # infeasible at T=7 -> skip
    net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=len(Ts), reg=0.01)
    costs, _, skips = net.costAndGradBatch(datas, labs, reg_in_grad=False)
    g_sync = net.grad.flat.clone()
    net.grad.flat.zero_()
    cost_dev, skip_dev = net.costAndGradBatchAsync(datas, labs, reg_in_grad=False)
    net.checkAsync()
    np.testing.assert_array_equal(skip_dev.cpu().numpy().astype(bool), skips)
    np.testing.assert_array_equal(cost_dev.cpu().numpy()[~skips], costs[~skips])
    assert torch.equal(net.grad.flat, g_sync)
    # without the L2 term in the gradient; with it the difference is reg * W on the weights only
    net.costAndGradBatch(datas, labs, reg_in_grad=True)
    diff = (net.grad.flat - g_sync).cpu().numpy()
    want = 0.01 * net._params.cpu().numpy()
    for lo, hi in net.noreg_ranges().reshape(-1, 2):
        want[lo:hi] = 0.0                                           # biases carry no L2 term
    # difference of two fp32 gradients of magnitude ~10: a few ulps of THEM, not of reg * W
    np.testing.assert_allclose(diff, want, rtol=1e-4, atol=2e-5)
    buckets = net.gradBuckets()
    assert all(ev for ev, _, _ in buckets)
    spans = sorted((s, e) for _, s, e in buckets)
    assert spans[0][0] == 0 and spans[-1][1] == net.grad.flat.numel()
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))     # exact cover, no overlap
    assert buckets[0][1] == int(net._infos[2 * NL].offset)          # output layer first (brnnet.py:191-193)
    assert [s for _, s, _ in buckets].index(int(net._infos[2 * (NL + 1)].offset)) == NL - TL + 1   # Wf right after the temporal layer
    assert net.regCostDev().item() == pytest.approx(net.regcost, rel=1e-6)   # engine: fp32 partial sums


@pytest.mark.parametrize("H,B,equal", [(512, 24, False), (1824, 32, False), (1824, 32, True), (2048, 17, False)])
def test_two_chain_recurrence_exchange_layout_is_bit_identical(mods, monkeypatch, H, B, equal):
    """17..32 utterances (brnn_recurrent_q_kernel): a tile's KB of the exchange buffer is kept in lane order while all 16
    utterances of the tile are alive and row-major for its last steps (round 5; a wave's load is one contiguous KB
    instead of 16-byte pieces 64 bytes apart: 6.8 -> 6.3 us per step at the headline shape).  Every lane receives the
    same values either way: costs and gradients are bit for bit those of SCTC_REC_VARIANT=46 (row-major throughout);
    ragged lengths switch a tile from one layout to the other in mid-pass, B = 17 leaves the second tile incomplete"""
    _, brnnet, obrnn, torch = mods
    rs = np.random.RandomState(H + B)
    D, A, NL, TL, Tmax = 24, 33, 3, 2, 14
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    Ts = [Tmax] * B if equal else [int(t) for t in rs.randint(1, Tmax + 1, size=B)]
    Ts[3] = Tmax
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 5)).astype(np.int32) for T in Ts]
    res = []
    for variant in ("0", "46"):
        monkeypatch.setenv("SCTC_REC_VARIANT", variant)
        net = make_net(brnnet, (D, A, H, NL, TL, Tmax), params, maxUtts=B)
        costs, _, skips = net.costAndGradBatch(datas, labs)
        assert net.recurrentPath()[0] == 1
        res.append((costs.copy(), skips.copy(), [net.grad[i][0].copy_to_host().copy() for i in range(NL + 3)]))
        del net
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2], res[1][2]):
        np.testing.assert_array_equal(a, b)
    if H <= 512:
        with np.errstate(all="ignore"):
            cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
        ok = ~sr
        np.testing.assert_allclose(res[0][0][ok], cr[ok], rtol=1e-4)
        assert rel(res[0][2][NL + 1], gr["Wf"]) < 2e-3


@pytest.mark.parametrize("H,B", [(512, 52), (1824, 64), (2048, 100), (96, 90), (512, 128)])
def test_large_minibatch_recurrence_pipelined_is_bit_identical(mods, monkeypatch, H, B):
    """more than 32 utterances on the one-slab-per-CU kernel (brnn_recurrent_kernel<NTW>; the default up to round 5, since
    round 6 SCTC_REC_VARIANT=47 and every layer size without the tiled form): round 5 issues the exchange loads of batch
    k+1 under the MFMAs of batch k; the same MFMAs on the same accumulators in the same order, so costs and every gradient
    are bit for bit what SCTC_REC_VARIANT=40 (loads, fence, MFMAs: rounds 1-4) gives; ragged lengths, both passes.
    The exchange layout: a tile of 16 utterances is kept [k quarter][utterance][4 units] (a wave reads one contiguous KB)
    while all 16 are alive and row-major for its last steps -- the ragged lengths here switch every tile from one to the
    other; SCTC_REC_VARIANT=46 keeps row-major throughout in whatever kernel the default is: same numbers as the default.
    Default (round 6: the units x utterances kernel where the layer size has one) against variant 47: another K split,
    so close, not equal."""
    _, brnnet, obrnn, torch = mods
    rs = np.random.RandomState(H + B)
    D, A, NL, TL, Tmax = 24, 33, 3, 2, 14
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    Ts = [int(t) for t in rs.randint(1, Tmax + 1, size=B)]
    Ts[3] = Tmax
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 5)).astype(np.int32) for T in Ts]
    res = []
    for variant in ("0", "46", "47", "40"):
        monkeypatch.setenv("SCTC_REC_VARIANT", variant)
        net = make_net(brnnet, (D, A, H, NL, TL, Tmax), params, maxUtts=B)
        costs, _, skips = net.costAndGradBatch(datas, labs)
        assert net.recurrentPath()[0] == 1
        res.append((costs.copy(), skips.copy(), [net.grad[i][0].copy_to_host().copy() for i in range(NL + 3)]))
        del net
    for first, other in ((res[0], res[1]), (res[2], res[3])):
        np.testing.assert_array_equal(first[0], other[0])
        np.testing.assert_array_equal(first[1], other[1])
        for a, b in zip(first[2], other[2]):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res[0][1], res[2][1])
    ok = ~res[0][1]
    np.testing.assert_allclose(res[0][0][ok], res[2][0][ok], rtol=1e-5)
    for a, b in zip(res[0][2], res[2][2]):
        assert rel(a, b) < 1e-3
    if H <= 512:
        with np.errstate(all="ignore"):
            cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
        ok = ~sr
        np.testing.assert_allclose(res[0][0][ok], cr[ok], rtol=1e-4)
        assert rel(res[0][2][NL + 1], gr["Wf"]) < 2e-3


@pytest.mark.parametrize("H,B", [(512, 4), (512, 5), (1824, 4), (2048, 5), (1024, 3)])
def test_recurrent_small_batch_crossover(mods, monkeypatch, H, B):
    """1..3 utterances run the sentinel / VALU kernel, 4 and 5 the single-chain flag kernel since round 5 (a step of the
    VALU kernel grows by 1 us per utterance: 4.9 / 7.0 us at 4 / 5 against 4.6 / 4.5): the default against the VALU
    kernel forced up to 8 utterances (SCTC_REC_VARIANT=43), the flag kernel forced from 1 (44) and, at H=512, the
    oracle; ragged lengths"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(7 * H + B)
    D, A, NL, TL = 32, 33, 2, 1
    Ts = [int(t) for t in rs.randint(2, 26, size=B)]
    Ts[0] = 26
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 8)).astype(np.int32) for T in Ts]
    res = {}
    for variant in ("0", "43", "44"):
        monkeypatch.setenv("SCTC_REC_VARIANT", variant)
        net = make_net(brnnet, (D, A, H, NL, TL, max(Ts)), params, maxUtts=B)
        costs, _, skips = net.costAndGradBatch(datas, labs)
        assert net.recurrentPath()[:2] == (1, 1)
        res[variant] = (costs.copy(), skips.copy(), _all_grads(net, NL))
        if variant == "0" and H == 512:
            with np.errstate(all="ignore"):
                costs_ref, g_ref, skips_ref, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
            np.testing.assert_array_equal(skips, skips_ref)
            np.testing.assert_allclose(costs[~skips_ref], costs_ref[~skips_ref], rtol=1e-4)
            check_grads(net, g_ref, NL)
        del net
    ok = ~res["0"][1]
    for other in ("43", "44"):
        np.testing.assert_array_equal(res["0"][1], res[other][1])
        np.testing.assert_allclose(res["0"][0][ok], res[other][0][ok], rtol=1e-5)
        for a, b in zip(res["0"][2], res[other][2]):
            assert rel(a, b) < 2e-4
    same_as = "44" if B >= 4 else "43"           # which forced kernel IS the default at this size
    for a, b in zip(res["0"][2], res[same_as][2]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("H,B", [(512, 33), (512, 40), (1824, 48), (512, 66), (1824, 80), (96, 40), (96, 70), (1024, 96)])
def test_recurrence_33_to_48_utterances_as_two_launches(mods, monkeypatch, H, B):
    """Minibatches cut into several launches (round 5: 33..48 as 32 + the rest, 65..80 as 64 + the rest; round 6, where the
    layer size has the units x utterances kernel: 33..64 in one launch, 65..96 as 64 + the rest -- recurrent.hip
    launch_recurrent): ragged lengths against a single launch (SCTC_REC_VARIANT=45) and, at H=512, the oracle"""
    _, brnnet, obrnn, _ = mods
    rs = np.random.RandomState(3 * H + B)
    D, A, NL, TL, Tmax = 24, 33, 3, 2, 18
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    Ts = [int(t) for t in rs.randint(1, Tmax + 1, size=B)]
    Ts[5] = Tmax
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 5)).astype(np.int32) for T in Ts]
    res = []
    for variant in ("0", "45"):
        monkeypatch.setenv("SCTC_REC_VARIANT", variant)
        net = make_net(brnnet, (D, A, H, NL, TL, Tmax), params, maxUtts=B)
        costs, _, skips = net.costAndGradBatch(datas, labs)
        assert net.recurrentPath()[0] == 1
        res.append((costs.copy(), skips.copy(), _all_grads(net, NL)))
        if variant == "0" and H <= 512:
            with np.errstate(all="ignore"):
                cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
            np.testing.assert_array_equal(skips, sr)
            np.testing.assert_allclose(costs[~sr], cr[~sr], rtol=1e-4)
            check_grads(net, gr, NL, tol=1e-3)      # (a boundary flip of one unit is within this: see test_recurrent_large_minibatch)
        del net
    ok = ~res[0][1]
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_allclose(res[0][0][ok], res[1][0][ok], rtol=1e-5)
    for a, b in zip(res[0][2], res[1][2]):
        assert rel(a, b) < 1e-3


def _note(text):      # observed numbers also go to gpurun_out/test_notes.txt (pytest swallows stdout)
    print(text)
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "test_notes.txt"), "a") as f:
            f.write(text + "\n")
    except OSError:
        pass


def _packed_rowbase(Ts):
    Ts = np.asarray(Ts)
    alive = np.array([(Ts > t).sum() for t in range(Ts.max())])
    return np.concatenate([[0], np.cumsum(alive)[:-1]])


@pytest.mark.parametrize("H,B,ragged", [(512, 33, True), (512, 64, False), (1024, 100, True), (1824, 64, True), (1824, 128, True),
                                        (2048, 128, False), (1824, 50, True), (512, 128, True)])
def test_tiled_recurrence_rows_equal_minibatches_of_32(mods, monkeypatch, H, B, ragged):
    """more than 32 utterances, round 6: brnn_recurrent_t_kernel (32 units x half the utterance tiles per CU, two
    alternating sub-chains, exchange loads in a register ring, the epilogue of a phase between the next phase's MFMAs)
    keeps the K split and the order of every addition of the two-chain kernel of 17..32 utterances, so the rows of
    hActsFor / hActsBack of an utterance are BIT-identical to what it gets in a minibatch of 32 (sorted order; the last,
    partial group of 1..16 runs other kernels and is left out); the whole step against the one-slab-per-CU kernel
    (SCTC_REC_VARIANT=47: another K split) and, at H=512, the oracle; run-to-run reproducible"""
    _, brnnet, obrnn, torch = mods
    rs = np.random.RandomState(5 * H + B)
    D, A, NL, TL, Tmax = 24, 33, 3, 2, 22
    Tmin = 2
    if H > 1024:        # enough frames that the GEMM in front of the recurrence runs without a K split in both minibatches
        Tmax, Tmin = 480, 455
    params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
    Ts = sorted([int(t) for t in (rs.randint(Tmin, Tmax + 1, size=B) if ragged else [Tmax] * B)], reverse=True)
    Ts[0] = Tmax
    datas = [rs.randn(D, T) for T in Ts]
    labs = [rs.randint(1, A, size=max(1, T // 5)).astype(np.int32) for T in Ts]
    # the tiled kernel is the default where it is faster (H >= 1824: 228 / 256 workgroups); at the small layer sizes of this
    # test it exists too (64 / 128 workgroups, no faster than the one-slab-per-CU kernel) and runs when asked for
    monkeypatch.setenv("SCTC_REC_VARIANT", "0" if H >= 1824 else "50")
    net = make_net(brnnet, (D, A, H, NL, TL, Tmax), params, maxUtts=B)
    costs, _, skips = net.costAndGradBatch(datas, labs)
    assert net.recurrentPath()[:2] == (1, 1)
    hF, hB, Z = net.debugBuffer(100), net.debugBuffer(101), net.debugBuffer(102)
    g_t = _all_grads(net, NL)
    net.costAndGradBatch(datas, labs)
    for a, b in zip(g_t, _all_grads(net, NL)):
        np.testing.assert_array_equal(a, b)
    if H == 512:
        with np.errstate(all="ignore"):
            cr, gr, sr, _ = obrnn.cost_and_grad_batch(params, datas, labs, TL)
        np.testing.assert_array_equal(skips, sr)
        np.testing.assert_allclose(costs[~sr], cr[~sr], rtol=1e-4)
        check_grads(net, gr, NL, tol=1e-3)
    del net
    monkeypatch.setenv("SCTC_REC_VARIANT", "47")
    net1 = make_net(brnnet, (D, A, H, NL, TL, Tmax), params, maxUtts=B)
    costs1, _, skips1 = net1.costAndGradBatch(datas, labs)
    np.testing.assert_array_equal(skips, skips1)
    np.testing.assert_allclose(costs[~skips], costs1[~skips], rtol=1e-5)
    for a, b in zip(g_t, _all_grads(net1, NL)):
        assert rel(a, b) < 1e-3
    del net1
    monkeypatch.setenv("SCTC_REC_VARIANT", "0")
    rb = _packed_rowbase(Ts)
    n_equal = n_seen = 0
    for b0 in range(0, B, 32):
        b1 = min(b0 + 32, B)
        if b1 - b0 <= 16:
            continue
        sub = make_net(brnnet, (D, A, H, NL, TL, Tmax), params, maxUtts=b1 - b0)
        sub.costAndGradBatch(datas[b0:b1], labs[b0:b1])
        sF, sB, sZ = sub.debugBuffer(100), sub.debugBuffer(101), sub.debugBuffer(102)
        rbs = _packed_rowbase(Ts[b0:b1])
        for b in range(b0, b1):
            tt = np.arange(Ts[b])
            # the recurrence's input W h + b comes out of a time-batched GEMM whose block shape follows the number of
            # frames: where that already differs in the last bit between the two minibatches, "equal" is not defined
            if np.array_equal(Z[rb[tt] + b], sZ[rbs[tt] + b - b0]):
                np.testing.assert_array_equal(hF[rb[tt] + b], sF[rbs[tt] + b - b0])
                np.testing.assert_array_equal(hB[rb[tt] + b], sB[rbs[tt] + b - b0])
                n_equal += 1
            else:
                np.testing.assert_allclose(hF[rb[tt] + b], sF[rbs[tt] + b - b0], rtol=1e-4, atol=1e-5)
                np.testing.assert_allclose(hB[rb[tt] + b], sB[rbs[tt] + b - b0], rtol=1e-4, atol=1e-5)
            n_seen += 1
        del sub
    _note("tiled recurrence H=%d B=%d: %d of %d utterances with bit-identical inputs, their hActsFor / hActsBack rows bit-identical to a minibatch of 32"
         % (H, B, n_equal, n_seen))
    assert n_equal > 0



@pytest.mark.parametrize("T_b", [(5,), (3,), (5, 3)], ids=["contiguous5", "contiguous3", "gathered"])
def test_gradients_do_not_depend_on_the_frames_the_handle_was_sized_for(mods, T_b):
    """The split-K workspace is sized at create time from plans for K = max_frames (csrc/gemm_plan.h,
    brnn_splitk_floats), the launches plan again for their own K: a handle created for 8192 frames -- beyond the
    K >= 4096 rule of the 16-bit tile choice and 1024 times the launch's K -- gives the gradients, bit for bit, of one
    created for the 10 frames it needs.  One utterance pairs contiguous rows in the recurrent weight gradients, the
    ragged pair gathers them."""
    _sctc, brnnet, obrnn, torch = mods
    D, A, H, NL, TL = 20, 6, 64, 2, 1
    rs = np.random.RandomState(7)
    data = [rs.randn(D, T) for T in T_b]
    labels = [np.array([1, 2], dtype=np.int32)[:min(2, T)] for T in T_b]
    got = []
    for maxBatch in (5, 4096):
        np.random.seed(11)
        net = brnnet.NNet(D, A, H, NL, maxBatch, temporalLayer=TL, maxUtts=2)
        net.initParams()
        cost, _, skip = net.costAndGradBatch(data, labels)
        assert not skip.any()
        got.append((cost.copy(), net._grads.clone()))
        assert bool(torch.isfinite(got[-1][1]).all()) and float(got[-1][1].abs().max()) > 0
    assert np.array_equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])
