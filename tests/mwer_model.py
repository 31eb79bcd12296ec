"""A restatement in plain float64 of the MWER contract (include/sctc.h, ctc_torch.mwer_loss).

Utterance n has frames T_n and hypotheses k < K_n[n] <= K with label rows y_k (length U_k >= 0, labels in [0, C), none
equal to the blank) and errors W_k (float64, any unit the caller likes).

* ll_k = log P_ctc(y_k | x_n), float64: minus the cost the CTC kernels return for that label row over that utterance's
  probabilities.
* Real.  Hypothesis k is real when k < K_n[n], W_k is finite, the CTC call's skip is 0 and its cost is finite (here:
  ll_k is finite).  Everything else has weight 0 and is never read beyond that test; its labels are not validated.
* Active.  An utterance is active when T_n >= 2 and it has at least one real hypothesis.  An inactive utterance has
  loss 0 and gradient rows of exact zeros.  (One frame is the shape where the CTC kernels follow the reference to
  -log(p_blank + p_label) instead of the CTC loss; MWER over a one-frame utterance is of no use, so it is left out, not
  special-cased.)
* Weights.  m = max ll_k over the real ones; w_k = exp(scale * (ll_k - m)); Z = sum w_k in ascending k; P_k = w_k / Z;
  R = sum P_k W_k in ascending k, the expected error; Wbar = (sum W_k, ascending k) / (number of real hypotheses).
  Everything is float64.
* Loss.  loss_n = R - Wbar, or R alone with subtract_mean=False.  The baseline changes the value, never the gradient.
* Coefficients.  c_k = scale * P_k * (W_k - R): this is d loss_n / d ll_k.
* Gradient.  d loss_n / d input[t, n, c] = sum_k c_k * occ_k[t, c] for t < T_n, exact 0 for padded frames; occ_k = p -
  g_k is the occupancy of symbol c at frame t under hypothesis k.  Because sum_k c_k = 0 the p term cancels: the sum is
  the exact derivative both with respect to activations in front of a softmax and with respect to raw
  log-probabilities.

Two halves.  `utterance` goes from (ll, W, K_n, T_n, scale) to loss / coef / posterior in plain Python floats.  `oracle`
is the whole loss built from torch.nn.functional.ctc_loss on CPU float64 tensors (reduction="none", one call per rank),
the weights and the loss written in torch ops, with autograd through all of it; `loss_from_ll` is its middle part.

The keyword switches named ``mut_*`` each break one rule; tests/test_mwer_model_cpu.py shows that every one of them
changes a hand-worked case, so that a device that had the rule wrong could not pass against the model by accident."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MUTATIONS = ("mut_descending", "mut_baseline_in_grad", "mut_wbar_in_coef", "mut_nonreal_in_wbar", "mut_no_scale",
             "mut_one_frame")


def utterance(ll, W, K_n, T_n, scale, subtract_mean=True, mut_descending=False, mut_baseline_in_grad=False,
              mut_wbar_in_coef=False, mut_nonreal_in_wbar=False, mut_no_scale=False, mut_one_frame=False):
    """ll, W: K floats each (ll_k non-finite where the CTC call skipped or its cost was not finite).  Returns a dict:
    loss, expected (floats), coef, posterior (float64 [K]), real (bool [K]), active (bool)."""
    K = len(ll)
    ll = [float(v) for v in ll]
    W = [float(v) for v in W]
    real = [k < K_n and math.isfinite(W[k]) and math.isfinite(ll[k]) for k in range(K)]
    active = (T_n >= 2 or mut_one_frame) and any(real)
    out = dict(loss=0.0, expected=0.0, coef=np.zeros(K), posterior=np.zeros(K), real=np.zeros(K, dtype=bool),
               active=bool(active))
    if not active:
        return out
    ranks = [k for k in range(K) if real[k]]
    order = ranks[::-1] if mut_descending else ranks
    m = max(ll[k] for k in ranks)
    w = {k: math.exp(scale * (ll[k] - m)) for k in ranks}
    Z = 0.0
    for k in order:
        Z += w[k]
    P = {k: w[k] / Z for k in ranks}
    R = 0.0
    for k in order:
        R += P[k] * W[k]
    in_mean = [k for k in range(K) if k < K_n and math.isfinite(W[k])] if mut_nonreal_in_wbar else ranks
    wsum = 0.0
    for k in (in_mean[::-1] if mut_descending else in_mean):
        wsum += W[k]
    wbar = wsum / len(in_mean)
    loss = R - wbar if subtract_mean else R
    centre = wbar if mut_wbar_in_coef else (loss if mut_baseline_in_grad else R)
    for k in ranks:
        out["coef"][k] = (1.0 if mut_no_scale else scale) * P[k] * (W[k] - centre)
        out["posterior"][k] = P[k]
        out["real"][k] = True
    out["loss"], out["expected"] = loss, R
    return out


def batch(ll, W, K_n, T_n, scale, subtract_mean=True, **mut):
    """`utterance` over [N, K] arrays: dict of loss [N], expected [N], coef, posterior, real [N, K], active [N]"""
    rows = [utterance(ll[n], W[n], int(K_n[n]), int(T_n[n]), scale, subtract_mean, **mut) for n in range(len(ll))]
    return {key: np.array([r[key] for r in rows]) for key in rows[0]}


def loss_from_ll(ll, W, real, scale, subtract_mean=True):
    """the loss of ONE active utterance in torch ops: ll a float64 tensor [K] (autograd flows through it), W a list of
    floats, real a list of bools with at least one True"""
    ranks = [k for k in range(len(W)) if real[k]]
    m = max(float(ll[k].detach()) for k in ranks)
    w = {k: torch.exp(scale * (ll[k] - m)) for k in ranks}
    Z = 0.0
    for k in ranks:
        Z = Z + w[k]
    R = 0.0
    wsum = 0.0
    for k in ranks:
        R = R + w[k] / Z * W[k]
        wsum += W[k]
    return R - wsum / len(ranks) if subtract_mean else R


def reduce(losses, reduction):
    if reduction == "none":
        return losses
    return losses.sum() if reduction == "sum" else losses.mean()


def oracle(x64, hyps, U, W, T_n, K_n=None, blank=0, scale=1.0, reduction="mean", subtract_mean=True, logits=False,
           weight=None):
    """The whole loss on CPU float64 tensors.  x64 [T, N, C]; hyps [N, K, S] integers (garbage allowed wherever the
    contract does not read); U [N, K]; W [N, K]; T_n [N]; K_n [N] or None.  Returns (loss reduced and detached, the
    gradient with respect to x64 of (loss * weight).sum(), stats) where stats holds loglik (-inf where not real),
    real [N, K] and the unreduced losses [N]."""
    x = x64.detach().clone().requires_grad_()
    T, N, C = x.shape
    hyps = np.asarray(hyps)
    K, S = hyps.shape[1], hyps.shape[2]
    U = np.asarray(U, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64)
    T_n = np.asarray(T_n, dtype=np.int64)
    K_n = np.full(N, K, dtype=np.int64) if K_n is None else np.asarray(K_n, dtype=np.int64)
    lp = x.log_softmax(2) if logits else x
    read = (np.arange(K)[None, :] < K_n[:, None]) & np.isfinite(W) & (T_n >= 2)[:, None]
    il = torch.from_numpy(T_n)
    ll = []
    feasible = np.zeros((N, K), dtype=bool)
    for k in range(K):
        # the slots the contract does not read: an empty target in their place, the answer dropped below
        tl = torch.from_numpy(np.where(read[:, k], U[:, k], 0))
        tg = torch.from_numpy(np.where(np.arange(S)[None, :] < tl.numpy()[:, None], hyps[:, k, :], 0).astype(np.int64))
        if S == 0:
            tg = torch.zeros((N, 1), dtype=torch.int64)
        with torch.no_grad():
            plain = F.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=False)
        feasible[:, k] = torch.isfinite(plain).numpy()
        # zero_infinity: its backward gives the infeasible rows zeros where the plain one gives NaN; they are not real
        ll.append(-F.ctc_loss(lp, tg, il, tl, blank=blank, reduction="none", zero_infinity=True))
    ll = torch.stack(ll, dim=1)                                                         # [N, K]
    real = read & feasible
    losses = []
    for n in range(N):
        if T_n[n] >= 2 and real[n].any():
            losses.append(loss_from_ll(ll[n], [float(v) for v in W[n]], list(real[n]), scale, subtract_mean))
        else:
            losses.append(torch.zeros((), dtype=torch.float64))
    losses = torch.stack([v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=torch.float64) for v in losses])
    loss = reduce(losses, reduction)
    total = (loss if weight is None else loss * weight).sum()
    if total.requires_grad:
        total.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    active = (T_n >= 2) & real.any(axis=1)
    real = real & active[:, None]
    loglik = np.where(real, ll.detach().numpy(), -np.inf)
    return loss.detach(), grad, dict(loglik=loglik, real=real, losses=losses.detach().numpy())
