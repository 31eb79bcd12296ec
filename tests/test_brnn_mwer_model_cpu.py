"""tests/brnn_mwer_model.py, the float64 restatement the GPU tests of the MWER step compare against, checked on the CPU:
against oracle/brnn.py (forward pass and CTC gradients), against the linearity of the backward pass, that every mutation
switch changes a case, and that no case of the GPU tests sits on a kink."""
import numpy as np
import pytest
import torch

from oracle import brnn as obrnn
from tests import brnn_mwer_model as bm
from tests import mwer_model


@pytest.fixture(scope="module")
def cases():
    return bm.cases()


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def grads_close(got, want, tol):
    worst = 0.0
    for a, b in zip(got["W"] + got["b"], want["W"] + want["b"]):
        worst = max(worst, rel(a, b))
    if want["Wf"] is not None:
        worst = max(worst, rel(got["Wf"], want["Wf"]), rel(got["Wb"], want["Wb"]))
    assert worst < tol, worst


@pytest.mark.parametrize("name", ["b3_k2", "tl0_reg", "a300_lam1"])
def test_forward_and_ctc_gradients_agree_with_the_oracle(cases, name):
    c = cases[name]
    for b in range(len(c.data)):
        P = bm.to_torch(c.params)
        logits, _ = bm.forward(P, c.data[b], c.TL)
        want, _ = obrnn.forward(c.params, c.data[b], c.TL, max_act=bm.MAX_ACT)
        np.testing.assert_allclose(logits.detach().numpy(), want, rtol=1e-12, atol=1e-12)
        cost, ok = bm.ctc_cost(logits, c.labels[b])
        assert ok
        cost.backward()
        c_ref, g_ref, skip, _ = obrnn.cost_and_grad(c.params, c.data[b], c.labels[b], c.TL, max_act=bm.MAX_ACT)
        assert not skip and float(cost.detach()) == pytest.approx(c_ref, rel=1e-11)
        got = {"W": [w.grad.numpy() for w in P["W"]], "b": [v.grad.numpy() for v in P["b"]],
               "Wf": None if P["Wf"] is None else P["Wf"].grad.numpy(), "Wb": None if P["Wb"] is None else P["Wb"].grad.numpy()}
        grads_close(got, g_ref, 1e-9)


@pytest.mark.parametrize("name", ["b3_k2", "uniform_lam", "a300_lam1"])
def test_gradient_is_the_coefficient_weighted_sum_of_ctc_gradients(cases, name):
    """by linearity of the backward pass: - sum_k c_k grads_k + lambda grads_ref, grads from oracle.brnn.cost_and_grad"""
    c = cases[name]
    B, K = len(c.data), c.K
    ll = np.full((B, K), -np.inf)
    G = [[None] * K for _ in range(B)]
    for b in range(B):
        for k in range(K):
            cost, g, skip, _ = obrnn.cost_and_grad(c.params, c.data[b], c.hyps[b][k], c.TL, max_act=bm.MAX_ACT)
            if not skip and np.isfinite(cost):
                ll[b, k], G[b][k] = -cost, g
    W = np.array([e for e in c.errors])
    st = mwer_model.batch(ll, W, c.K_b, c.T_b, c.scale, c.subtract_mean)
    keys = ["W", "b"] + (["Wf", "Wb"] if c.params["Wf"] is not None else [])
    flat = lambda g: [m for key in keys for m in (g[key] if isinstance(g[key], list) else [g[key]])]
    total = None
    add = lambda tot, g, f: [f * m for m in flat(g)] if tot is None else [t + f * m for t, m in zip(tot, flat(g))]
    for b in range(B):
        for k in range(K):
            if st["real"][b, k]:
                total = add(total, G[b][k], -st["coef"][b, k])
        if c.ctc_weight > 0:
            cost, g, skip, _ = obrnn.cost_and_grad(c.params, c.data[b], c.labels[b], c.TL, max_act=bm.MAX_ACT)
            assert not skip
            total = add(total, g, c.ctc_weight)
    m = c.model()
    np.testing.assert_allclose(m["coef"], st["coef"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(m["posterior"], st["posterior"], rtol=1e-9, atol=1e-12)
    for got, want in zip(flat(m["grads"]), total):
        assert rel(got, want) < 1e-8


def changed(a, b):
    for key in ("loss", "expected", "posterior", "real", "inactive"):
        if not np.array_equal(np.nan_to_num(a[key], posinf=1e300), np.nan_to_num(b[key], posinf=1e300)):
            return True
    ga, gb = a["grads"], b["grads"]
    return any(rel(x, y) > 1e-6 for x, y in zip(ga["W"], gb["W"]) if np.linalg.norm(y) > 0)


@pytest.mark.parametrize("mut,name", [("mut_rank_order", "b3_k2"), ("mut_ref_in_posterior", "uniform_lam"),
                                      ("mut_empty_skipped", "ragged_empty_equal_lam"), ("mut_ref_skip_kept", "ref_skips"),
                                      ("mut_combine_sign", "b3_k2")])
def test_every_mutation_changes_a_case(cases, mut, name):
    assert mut in bm.MUTATIONS
    c = cases[name]
    assert changed(c.model(**{mut: True}), c.model())


def test_the_mutation_list_is_covered():
    assert set(bm.MUTATIONS) == {"mut_rank_order", "mut_ref_in_posterior", "mut_empty_skipped", "mut_ref_skip_kept",
                                 "mut_combine_sign"}


def test_no_case_of_the_gpu_tests_sits_on_a_kink(cases):
    for name, c in cases.items():
        assert c.model()["kink"] > 1e-5, name


def test_cases_hold_what_their_names_say(cases):
    m = cases["ragged_empty_equal_lam"].model()
    assert m["real"][0, 1] and len(cases["ragged_empty_equal_lam"].hyps[0][1]) == 0       # the empty hypothesis is real
    assert m["posterior"][0, 0] == pytest.approx(m["posterior"][0, 2], rel=1e-12)             # two equal hypotheses
    assert not m["real"][1, 1:].any() and not m["real"][2, 2]                                # beyond K_b
    m = cases["a70_k8_nan_long_scale"].model()
    assert not m["real"][1, 2] and not m["real"][0, 3] and not m["real"][2, 0] and m["real"].sum() == 21
    m = cases["one_frame"].model()
    assert list(m["inactive"]) == [False, True, False]
    assert cases["all_inactive"].model()["inactive"].all()
    m = cases["all_inactive_lam"].model()
    assert m["inactive"].all() and not m["ctc_skip"].any() and np.linalg.norm(m["grads"]["W"][0]) > 0
    m = cases["ref_skips"].model()
    assert list(m["ctc_skip"]) == [False, True, False]
    m = cases["k1"].model()
    assert all(np.all(g == 0) for g in m["grads"]["W"])                                      # K = 1: sum_k c_k = c_0 = 0
    m = cases["scale0"].model()
    assert np.allclose(m["posterior"], 1.0 / 3) and all(np.all(g == 0) for g in m["grads"]["W"])
