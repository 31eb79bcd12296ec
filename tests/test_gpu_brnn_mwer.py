"""The MWER step of the BRNN engine (NNet.mwerCostAndGradBatch, sctc_brnn_mwer_cost_and_grad) on the
device: against the float64 restatement tests/brnn_mwer_model.py, against the device's own CTC steps, and bit for bit
where the contract says so.  The minibatches are brnn_mwer_model.cases(): nets of the size of tests/golden/brnn_main.npz,
T <= 14, B <= 3.

Bounds against the float64 model start from the project's BRNN bounds (tests/test_gpu_brnn.py): loss and posterior 1e-4
relative where the model's value is not zero, expected 1e-4 * max(1, max |W|) absolute, every gradient tensor 1e-4
relative Frobenius norm where the model's tensor is not zero (exact zeros where it is); real and inactive equal.
Measured worst cases on an MI355X over the cases below: loss 1.81e-5 (b3_k2, where R - Wbar nearly cancels), posterior
1.30e-5 (scale = 30), expected 1.97e-7 absolute at max |W| = 5, gradients 2.24e-6; against the device's own CTC
gradients 2.68e-7.  Loss and posterior are not below an eighth of their bound and keep it; the others are tightened to
8 x the measured value: expected 3.2e-7 * max(1, max |W|), gradients 1.8e-5, self-consistency 2.2e-6."""
import os
import subprocess

import numpy as np
import pytest

from tests import brnn_mwer_model as bm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
TOL = 1e-4               # loss, posterior
TOL_EXPECTED = 3.2e-7    # times max(1, max |W|)
TOL_GRAD = 1.8e-5
TOL_SELF = 2.2e-6


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import _sctc
    from nnets import brnnet
    return _sctc, brnnet, torch


@pytest.fixture(scope="module")
def cases():
    return bm.cases()


@pytest.fixture(scope="module")
def models(cases):
    """the float64 model of every case, computed once and left unchanged"""
    memo = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in memo:
            memo[key] = cases[name].model(**kw)
        return memo[key]
    return get


def make_net(brnnet, c, fp16=False, reg=None, maxBatch=None):
    net = brnnet.NNet(c.D, c.A, c.H, c.NL, maxBatch or max(c.T_b), temporalLayer=c.TL, reg=c.reg if reg is None else reg,
                      maxUtts=len(c.T_b), fp16=fp16)
    net.setParams(c.host_stack())
    return net


def run(net, c, **kw):
    args = dict(labels_list=c.labels if c.ctc_weight > 0 else None, scale=c.scale, subtract_mean=c.subtract_mean,
                ctc_weight=c.ctc_weight, return_stats=True)
    args.update(kw)
    return net.mwerCostAndGradBatch(c.data, c.hyps, c.errors, **args)


def grads_of(net):
    """every gradient tensor as a float32 host copy: (name, array)"""
    NL = net.numLayers
    out = []
    for i in range(NL + 1):
        out.append(("W%d" % (i + 1), net.grad[i][0].copy_to_host().copy()))
        out.append(("b%d" % (i + 1), net.grad[i][1].copy_to_host().copy().reshape(-1, 1)))
    if net.temporalLayer > 0:
        out.append(("Wf", net.grad[NL + 1][0].copy_to_host().copy()))
        out.append(("Wb", net.grad[NL + 2][0].copy_to_host().copy()))
    return out


def model_grads(g):
    out = []
    for i, (w, b) in enumerate(zip(g["W"], g["b"])):
        out += [("W%d" % (i + 1), w), ("b%d" % (i + 1), np.asarray(b).reshape(-1, 1))]
    if g["Wf"] is not None:
        out += [("Wf", g["Wf"]), ("Wb", g["Wb"])]
    return out


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b)


def compare_grads(got, want, what, tol=TOL_GRAD, factor=1.0):
    worst = 0.0
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, g), (_, w) in zip(got, want):
        w = factor * np.asarray(w, dtype=np.float64)
        if np.linalg.norm(w) == 0.0:
            assert not np.any(g), (what, name)
            continue
        worst = max(worst, rel(g, w))
    print("%s: worst gradient error %.3g" % (what, worst))
    assert worst < tol, (what, worst)
    return worst


def compare_stats(loss, inactive, stats, m, c, what):
    assert np.array_equal(inactive, m["inactive"]), what
    assert np.array_equal(stats["real"], m["real"]), what
    assert np.array_equal(stats["ctc_skip"], m["ctc_skip"]), what
    wmax = max([1.0] + [abs(v) for e in c.errors for v in e if np.isfinite(v)])
    e_exp = np.abs(stats["expected"] - m["expected"]).max()
    nz = m["loss"] != 0
    e_loss = (np.abs(loss[nz] - m["loss"][nz]) / np.abs(m["loss"][nz])).max() if nz.any() else 0.0
    assert np.all(loss[~nz] == 0) or np.abs(loss[~nz]).max() <= TOL * wmax, what       # R - Wbar may cancel to zero
    nz = m["posterior"] != 0
    e_post = (np.abs(stats["posterior"][nz] - m["posterior"][nz]) / m["posterior"][nz]).max() if nz.any() else 0.0
    assert not np.any(stats["posterior"][~nz]), what
    print("%s: loss %.3g  expected %.3g  posterior %.3g" % (what, e_loss, e_exp, e_post))
    assert e_exp <= TOL_EXPECTED * wmax and e_loss <= TOL and e_post <= TOL, (what, e_loss, e_exp, e_post)


# ---------------------------------------------------------------- against the float64 model

@pytest.mark.parametrize("name", sorted(bm.cases()))
def test_against_the_float64_model(mods, cases, models, name):
    _sctc, brnnet, torch = mods
    c = cases[name]
    net = make_net(brnnet, c)
    loss, grad, inactive, stats = run(net, c)
    m = models(name)
    compare_stats(loss, inactive, stats, m, c, name)
    compare_grads(grads_of(net), model_grads(m["grads"]), name)
    if c.reg > 0:
        assert net.regcost > 0
        run(net, c, reg_in_grad=False)
        compare_grads(grads_of(net), model_grads(models(name, reg_in_grad=False)["grads"]), name + " reg_in_grad=False")


def test_accumulate_adds_the_step(mods, cases, models):
    _sctc, brnnet, torch = mods
    c = cases["uniform_lam"]
    net = make_net(brnnet, c)
    run(net, c)
    run(net, c, accumulate=True)
    compare_grads(grads_of(net), model_grads(models("uniform_lam")["grads"]), "accumulate", factor=2.0)


# ---------------------------------------------------------------- against the device's own CTC steps

@pytest.mark.parametrize("name", ["b3_k2", "uniform_lam", "a300_lam1"])
def test_gradient_is_the_weighted_sum_of_the_devices_ctc_gradients(mods, cases, name):
    """- sum_{b,k} c_{b,k} G_{b,k} + lambda sum_b G_ref_b, G from costAndGradBatch on utterance b with that label row;
    c = scale * P * (W - R) from the returned posterior and expected error"""
    _sctc, brnnet, torch = mods
    c = cases[name]
    net = make_net(brnnet, c)
    loss, grad, inactive, stats = run(net, c)
    got = grads_of(net)
    assert stats["real"].all()
    total = [np.zeros(g.shape, dtype=np.float64) for _, g in got]
    for b in range(len(c.data)):
        rows = [(-c.scale * stats["posterior"][b, k] * (c.errors[b][k] - stats["expected"][b]), c.hyps[b][k]) for k in range(c.K)]
        if c.ctc_weight > 0:
            rows.append((c.ctc_weight, c.labels[b]))
        for f, lab in rows:
            cost, _, skip = net.costAndGradBatch([c.data[b]], [lab])
            assert not skip[0]
            for t, (_, g) in zip(total, grads_of(net)):
                t += f * g.astype(np.float64)
    compare_grads(got, [(n, t) for (n, _), t in zip(got, total)], name + " self-consistency", tol=TOL_SELF)


# ---------------------------------------------------------------- exact

def same_bits(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, x), (_, y) in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, name)


def stats_bits(r):
    loss, _, inactive, stats = r
    return [loss, inactive, stats["expected"], stats["posterior"], stats["real"], stats["ctc_cost"], stats["ctc_skip"]]


def test_two_runs_are_bit_equal(mods, cases):
    _sctc, brnnet, torch = mods
    c = cases["ragged_empty_equal_lam"]
    net = make_net(brnnet, c)
    r1, g1 = run(net, c), None
    g1 = grads_of(net)
    r2 = run(net, c)
    same_bits(g1, grads_of(net), "two runs")
    for x, y in zip(stats_bits(r1), stats_bits(r2)):
        assert np.array_equal(x, y, equal_nan=True)


def test_one_hypothesis_gives_exact_zero_gradients(mods, cases):
    _sctc, brnnet, torch = mods
    c = cases["k1"]
    net = make_net(brnnet, c)
    net.grad.flat.fill_(7.0)
    loss, _, inactive, stats = run(net, c)
    assert not inactive[0] and stats["posterior"][0, 0] == 1.0 and loss[0] == 0.0
    for name, g in grads_of(net):
        assert not np.any(g), name


def test_padding_slots_change_nothing(mods, cases):
    _sctc, brnnet, torch = mods
    c = cases["ragged_empty_equal_lam"]
    net = make_net(brnnet, c)
    r1 = run(net, c)
    g1 = grads_of(net)
    Kp = 5
    junk = np.array([999, -4, 0, 123456] * 9, dtype=np.int32)          # labels outside the alphabet, longer than the frames
    hyps = [list(h) + [junk] * (Kp - len(h)) for h in c.hyps]
    errs = [np.concatenate([e, np.full(Kp - len(e), np.nan)]) for e in c.errors]
    r2 = net.mwerCostAndGradBatch(c.data, hyps, errs, labels_list=c.labels, scale=c.scale, ctc_weight=c.ctc_weight,
                                  return_stats=True, _K=Kp, _K_b=c.K_b)
    same_bits(g1, grads_of(net), "padding")
    a, b = stats_bits(r1), stats_bits(r2)
    for i, (x, y) in enumerate(zip(a, b)):
        if x.ndim == 2:
            assert not np.any(y[:, c.K:])
            y = y[:, :c.K]
        assert np.array_equal(x, y, equal_nan=True), i
    # a non-finite error inside K_b takes the slot out in the same way, garbage labels and all
    r3 = net.mwerCostAndGradBatch(c.data, hyps, errs, labels_list=c.labels, scale=c.scale, ctc_weight=c.ctc_weight,
                                  return_stats=True)
    same_bits(g1, grads_of(net), "NaN errors")
    assert np.array_equal(r1[0], r3[0])


def test_labels_are_not_read_without_a_ctc_weight(mods, cases):
    _sctc, brnnet, torch = mods
    c = cases["b3_k2"]
    net = make_net(brnnet, c)
    r1 = run(net, c, labels_list=None)
    g1 = grads_of(net)
    r2 = run(net, c, labels_list=[np.array([999999], dtype=np.int32)] * 3)
    same_bits(g1, grads_of(net), "labels with ctc_weight = 0")
    assert np.array_equal(r1[0], r2[0]) and not r2[3]["ctc_skip"].any() and not r2[3]["ctc_cost"].any()


@pytest.fixture(scope="module")
def plan_query(tmp_path_factory):
    """the kernels csrc/ctc_plan.h names for a call, under this process's (unset) switches"""
    exe = str(tmp_path_factory.mktemp("ctc_plan") / "ctc_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "ctc_plan_dump.cpp"), "-o", exe])

    def query(B, A, max_L, max_T):
        out = subprocess.run([exe, "query"], input="%d %d 0 %d %d\n" % (B, A, max_L, max_T), stdout=subprocess.PIPE,
                             universal_newlines=True, check=True).stdout
        return [line.strip() for line in out.splitlines() if line.strip() != "end"]
    return query


@pytest.mark.parametrize("name", ["b3_k2", "uniform_lam"])
def test_one_hypothesis_and_unit_ctc_weight_is_the_ctc_step(mods, cases, plan_query, name):
    """K = 1, lambda = 1: the hypothesis' coefficient is exactly 0, what is left is g_ref -- bit-equal to costAndGradBatch
    on the references where both CTC batches (B rows there, 2 B rows here) run the same kernel"""
    for k in os.environ:
        assert not k.startswith("SCTC_CTC_"), "natural dispatch: %s is set" % k
    _sctc, brnnet, torch = mods
    c = cases[name]
    B = len(c.data)
    hyps, errs = [[h[0]] for h in c.hyps], [e[:1] for e in c.errors]
    max_L = 2 * max(len(l) for l in c.labels + [h[0] for h in hyps]) + 1
    same_kernel = plan_query(2 * B, c.A, max_L, max(c.T_b)) == plan_query(B, c.A, 2 * max(len(l) for l in c.labels) + 1, max(c.T_b))
    net = make_net(brnnet, c)
    cost, _, skip = net.costAndGradBatch(c.data, c.labels)
    want = grads_of(net)
    loss, _, inactive, stats = net.mwerCostAndGradBatch(c.data, hyps, errs, labels_list=c.labels, ctc_weight=1.0,
                                                        return_stats=True)
    got = grads_of(net)
    assert not skip.any() and not stats["ctc_skip"].any()
    np.testing.assert_allclose(stats["ctc_cost"], cost, rtol=1e-12)
    np.testing.assert_allclose(loss, cost, rtol=1e-12)              # R - Wbar = 0 with one hypothesis
    if same_kernel:
        same_bits(want, got, name)
    else:
        compare_grads(got, [(n, g.astype(np.float64)) for n, g in want], name + " (different CTC kernels)")


def test_no_stale_state_between_ctc_and_mwer_steps(mods, cases):
    _sctc, brnnet, torch = mods
    c = cases["ragged_empty_equal_lam"]
    rs = np.random.RandomState(99)
    long_data = [rs.randn(c.D, 14) for _ in range(3)]
    long_labels = [rs.randint(1, c.A, size=5).astype(np.int32) for _ in range(3)]
    fresh = make_net(brnnet, c, maxBatch=14)
    run(fresh, c)
    mwer_fresh = grads_of(fresh)
    fresh2 = make_net(brnnet, c, maxBatch=14)
    fresh2.costAndGradBatch(long_data, long_labels)
    ctc_fresh = grads_of(fresh2)
    net = make_net(brnnet, c, maxBatch=14)
    net.costAndGradBatch(long_data, long_labels)
    run(net, c)
    same_bits(mwer_fresh, grads_of(net), "MWER after a longer CTC step")
    net.costAndGradBatch(long_data, long_labels)
    same_bits(ctc_fresh, grads_of(net), "CTC after an MWER step")


def test_an_inactive_utterance_leaves_zero_rows(mods, cases):
    """dlogits persists between steps: after a CTC step filled its rows, a minibatch of one inactive utterance must give
    an output-layer bias gradient (the column sums of dlogits) of exact zeros"""
    _sctc, brnnet, torch = mods
    c = cases["all_inactive"]
    net = make_net(brnnet, c)
    net.costAndGradBatch(c.data, c.labels)
    assert np.any(net.grad[c.NL][1].copy_to_host())
    loss, _, inactive, stats = net.mwerCostAndGradBatch(c.data[:1], c.hyps[:1], c.errors[:1], return_stats=True)
    assert inactive[0] and loss[0] == 0.0 and not stats["real"].any()
    for name, g in grads_of(net):
        assert not np.any(g), name
    one = bm.cases()["one_frame"]
    net = make_net(brnnet, one)
    net.costAndGradBatch(one.data, one.labels)
    loss, _, inactive, _ = net.mwerCostAndGradBatch(one.data[1:2], one.hyps[1:2], one.errors[1:2], return_stats=True)
    assert inactive[0] and not np.any(net.grad[one.NL][1].copy_to_host())


# ---------------------------------------------------------------- other

def test_fp16_operands(mods, cases):
    """the 16-bit-operand configuration against the fp32 engine at the tolerance tests/test_gpu_fp16.py states for the
    configuration: cost 2e-3 relative, gradients 5e-2 relative Frobenius norm"""
    _sctc, brnnet, torch = mods
    c = cases["uniform_lam"]
    net = make_net(brnnet, c)
    loss, _, _, stats = run(net, c)
    want = grads_of(net)
    net16 = make_net(brnnet, c, fp16=True)
    loss16, _, inactive16, stats16 = run(net16, c)
    assert not inactive16.any() and stats16["real"].all()
    np.testing.assert_allclose(stats16["ctc_cost"], stats["ctc_cost"], rtol=2e-3)
    compare_grads(grads_of(net16), [(n, g.astype(np.float64)) for n, g in want], "fp16 operands", tol=5e-2)


def test_async_entry_gives_the_same_bits(mods, cases):
    _sctc, brnnet, torch = mods
    c = cases["uniform_lam"]
    net = make_net(brnnet, c)
    r = run(net, c)
    g = grads_of(net)
    res = net.mwerCostAndGradBatchAsync(c.data, c.hyps, c.errors, labels_list=c.labels, scale=c.scale, ctc_weight=c.ctc_weight)
    net.checkAsync()
    same_bits(g, grads_of(net), "async")
    assert np.array_equal(res["loss"].cpu().numpy(), r[0]) and np.array_equal(res["posterior"].cpu().numpy(), r[3]["posterior"])
    assert np.array_equal(res["inactive"].cpu().numpy().astype(bool), r[2])


def test_workspace_is_required(mods, cases):
    _sctc, brnnet, torch = mods
    import ctypes
    c = cases["b3_k2"]
    net = make_net(brnnet, c)
    run(net, c)
    L = _sctc.lib()
    _sctc.check(L.sctc_brnn_set_mwer_workspace(net._h, None, 0))
    net._grow_mwer_workspace = lambda mb, mw: None
    with pytest.raises(_sctc.SctcError, match="workspace"):
        run(net, c)
    with pytest.raises(ValueError, match="outside"):
        net.mwerCostAndGradBatch(c.data, [[np.array([0, 1])]] * 3, [np.zeros(1)] * 3)       # the blank in a hypothesis


def test_nbest_batch_is_the_calls_made_by_hand(mods, cases):
    _sctc, brnnet, torch = mods
    import ctc_fast
    c = cases["uniform_lam"]
    net = make_net(brnnet, c)
    hyps, errs = net.nbestBatch(c.data, c.labels, 4, beam=8, unit="char")
    lp, T_b = net.forwardDevice(c.data, log=True)
    rows, scores = ctc_fast.decode_beam_batch(lp, [int(t) for t in T_b], beam=8, nbest=4)
    for b in range(3):
        keep = [k for k in range(4) if scores[b, k] != float("-inf")]
        assert len(hyps[b]) == len(keep) >= 1
        for h, k in zip(hyps[b], keep):
            assert np.array_equal(h, np.asarray(rows[b][k], dtype=np.int32))
        want = ctc_fast.edit_distance_batch([np.asarray(c.labels[b], dtype=np.int32)] * len(keep),
                                            [np.asarray(h, dtype=np.int32) for h in hyps[b]])[:, 0]
        assert np.array_equal(errs[b], want.astype(np.float64))
    space = 1
    hw, ew = net.nbestBatch(c.data, c.labels, 2, beam=8, unit="word", space=space)
    flat = [h for row in hw for h in row]
    owner = [b for b, row in enumerate(hw) for _ in row]
    want = ctc_fast.word_errors_batch([np.asarray(c.labels[b], dtype=np.int32) for b in owner], flat, space, A=c.A)[:, 0]
    assert np.array_equal(np.concatenate(ew), want.astype(np.float64))


def test_one_sgd_step_lowers_the_expected_error(mods, cases):
    _sctc, brnnet, torch = mods
    import sgd
    c = cases["uniform_lam"]
    net = make_net(brnnet, c)
    opts = dict(nbest=4, beam=8, unit="char", scale=1.0)
    hyps, errs = net.nbestBatch(c.data, c.labels, 4, beam=8, unit="char")
    assert max(len(h) for h in hyps) >= 2 and any(np.ptp(e) > 0 for e in errs)
    before = net.mwerCostAndGradBatch(c.data, hyps, errs, return_stats=True)[3]["expected"]
    opt = sgd.SGD(net, max(c.T_b), alpha=1e-3, momentum=0.0, minibatch=3, criterion="mwer", mwer=opts)
    opt.it = 1
    opt._step([(b, c.data[b], np.asarray(c.labels[b], dtype=np.int32)) for b in range(3)], 10, 0.0)
    assert opt.last_expected == pytest.approx(float(before.mean()), rel=1e-6)
    after = net.mwerCostAndGradBatch(c.data, hyps, errs, return_stats=True)[3]["expected"]
    assert after.sum() < before.sum(), (before, after)
