"""tests/mwer_model.py against hand-worked cases (no GPU): the rules of DESIGN.md §4.16 one by one, every mutation
switch shown to change at least one case, and the model's two halves held against each other -- autograd's
d loss / d ll_k through the torch half equals the plain half's c_k."""
import math

import numpy as np
import pytest
import torch

from tests import mwer_model as mm

INF = float("inf")
NAN = float("nan")

# name: (ll, W, K_n, T_n, scale, subtract_mean)
CASES = {
    "equal_pair": ([-3.0, -3.0], [0.0, 2.0], 2, 5, 0.7, True),
    "four_to_one": ([-1.0, -1.0 - math.log(4.0) / 2.0, -0.5], [1.0, 3.0, 100.0], 2, 9, 2.0, True),
    "four_to_one_raw": ([-1.0, -1.0 - math.log(4.0) / 2.0, -0.5], [1.0, 3.0, 100.0], 2, 9, 2.0, False),
    "infeasible_middle": ([-1.0, -INF, -1.0], [0.0, 6.0, 2.0], 3, 4, 1.0, True),
    "big_and_small": ([-2.0, -2.0, -2.0], [1e16, 1.0, 1.0], 3, 3, 1.0, True),
    "one_frame": ([-1.0, -2.0], [1.0, 0.0], 2, 1, 1.0, True),
    "nan_error": ([-1.0, -1.0, -1.0], [NAN, 1.0, 5.0], 3, 6, 3.0, True),
    "nothing_real": ([-INF, -1.0], [1.0, INF], 2, 6, 1.0, True),
}


def run(name, **mut):
    ll, W, K_n, T_n, scale, sub = CASES[name]
    return mm.utterance(ll, W, K_n, T_n, scale, sub, **mut)


def test_equal_pair():
    r = run("equal_pair")
    assert r["active"] and list(r["real"]) == [True, True]
    assert list(r["posterior"]) == [0.5, 0.5] and r["expected"] == 1.0 and r["loss"] == 0.0
    assert list(r["coef"]) == [-0.35, 0.35]


def test_four_to_one_and_the_rank_beyond_the_count():
    r = run("four_to_one")
    assert list(r["real"]) == [True, True, False]
    np.testing.assert_allclose(r["posterior"], [0.8, 0.2, 0.0], rtol=1e-15)
    assert r["expected"] == pytest.approx(1.4, rel=1e-15) and r["loss"] == pytest.approx(-0.6, rel=1e-14)
    np.testing.assert_allclose(r["coef"], [-0.64, 0.64, 0.0], rtol=1e-14)
    assert r["coef"][2] == 0.0 and not np.signbit(r["coef"][2])
    raw = run("four_to_one_raw")
    assert raw["loss"] == raw["expected"] == r["expected"]
    assert np.array_equal(raw["coef"], r["coef"])           # the baseline changes the value, never the gradient


def test_ranks_that_are_not_real():
    r = run("infeasible_middle")
    assert list(r["real"]) == [True, False, True]
    assert list(r["posterior"]) == [0.5, 0.0, 0.5] and r["expected"] == 1.0 and r["loss"] == 0.0       # Wbar = 2 / 2
    assert list(r["coef"]) == [-0.5, 0.0, 0.5]
    r = run("nan_error")
    assert list(r["real"]) == [False, True, True]
    assert r["expected"] == 3.0 and r["loss"] == 0.0 and list(r["coef"]) == [0.0, -3.0, 3.0]


def test_inactive_utterances():
    for name in ("one_frame", "nothing_real"):
        r = run(name)
        assert not r["active"] and r["loss"] == 0.0 and r["expected"] == 0.0
        assert not r["coef"].any() and not r["posterior"].any() and not r["real"].any()


def test_the_coefficients_sum_to_zero():
    rs = np.random.RandomState(0)
    for _ in range(20):
        K = int(rs.randint(1, 9))
        r = mm.utterance(-5 * rs.rand(K), rs.randint(0, 9, size=K).astype(float), K, 7, float(rs.choice([0.5, 1.0, 5.0])))
        assert abs(r["coef"].sum()) <= 1e-14 * max(1.0, np.abs(r["coef"]).max())
        assert r["posterior"].sum() == pytest.approx(1.0, rel=1e-15)


@pytest.mark.parametrize("mut", mm.MUTATIONS)
def test_every_switch_changes_a_case(mut):
    changed = []
    for name in CASES:
        a, b = run(name), run(name, **{mut: True})
        same = all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
        if not same:
            changed.append(name)
    assert changed, "%s changes no hand-worked case" % mut


def test_switches_are_the_model_s_keywords():
    import inspect
    params = inspect.signature(mm.utterance).parameters
    assert [p for p in params if p.startswith("mut_")] == list(mm.MUTATIONS)


@pytest.mark.parametrize("subtract_mean", [True, False])
@pytest.mark.parametrize("scale", [0.0, 0.5, 1.0, 5.0])
def test_the_two_halves_agree(scale, subtract_mean):
    rs = np.random.RandomState(int(scale * 10) + subtract_mean)
    for _ in range(10):
        K = int(rs.randint(1, 9))
        ll = -6.0 * rs.rand(K)
        W = rs.randint(0, 12, size=K).astype(np.float64)
        if K > 2:
            ll[rs.randint(K)] = -INF
            W[rs.randint(K)] = INF
        K_n = int(rs.randint(max(1, K - 1), K + 1))
        plain = mm.utterance(ll, W, K_n, 5, scale, subtract_mean)
        if not plain["active"]:
            continue
        t = torch.tensor(np.where(np.isfinite(ll), ll, 0.0), dtype=torch.float64, requires_grad=True)
        loss = mm.loss_from_ll(t, list(W), list(plain["real"]), scale, subtract_mean)
        loss.backward()
        bound = 1e-12 * max(1.0, scale * W[plain["real"]].max())
        assert abs(loss.item() - plain["loss"]) <= bound
        assert np.abs(t.grad.numpy() - plain["coef"]).max() <= bound


def test_oracle_against_finite_differences_and_the_plain_half():
    rs = np.random.RandomState(3)
    T, N, K, C = 5, 2, 3, 4
    hyps = np.array([[[1, 2], [3, 0], [2, 2]], [[1, 0], [-7, 99], [3, 1]]])
    U = np.array([[2, 1, 2], [1, 2, 2]])
    W = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0]])
    T_n, K_n = [5, 4], [3, 3]
    W[1, 1] = INF               # its labels are garbage and must not be read
    for logits in (True, False):
        x = torch.from_numpy(rs.randn(T, N, C))
        x = x if logits else x.log_softmax(2)
        loss, grad, st = mm.oracle(x, hyps, U, W, T_n, K_n, scale=1.5, reduction="sum", logits=logits)
        assert st["real"].tolist() == [[True, True, True], [True, False, True]]
        plain = mm.batch(st["loglik"], W, K_n, T_n, 1.5)
        assert plain["loss"].sum() == pytest.approx(loss.item(), rel=1e-12)
        assert not grad[4:, 1].any()
        num = torch.zeros_like(x)
        for i in range(x.numel()):
            for sgn in (1.0, -1.0):
                y = x.clone().reshape(-1)
                y[i] += sgn * 1e-6
                v, _, _ = mm.oracle(y.reshape(x.shape), hyps, U, W, T_n, K_n, scale=1.5, reduction="sum", logits=logits)
                num.reshape(-1)[i] += sgn * v.item() / 2e-6
        # in both modes: sum_k c_k = 0 cancels the p term of the CTC gradient, so the raw log-probabilities' derivative
        # is the same sum
        np.testing.assert_allclose(grad.numpy(), num.numpy(), rtol=1e-5, atol=1e-7)
