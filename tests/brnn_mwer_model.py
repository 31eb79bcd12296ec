"""A float64 restatement in torch, on the CPU, of the BRNN engine's MWER step (include/sctc.h,
NNet.mwerCostAndGradBatch).

The forward pass is oracle/brnn.py's (ReLU layers, one bidirectional recurrence clipped to [0, max_act], softmax)
written in torch ops; on top of it torch.nn.functional.ctc_loss gives the log-likelihood of every hypothesis and of the
reference, tests/mwer_model.loss_from_ll the MWER loss, and the step's objective is

    sum_b  loss_b  +  ctc_weight * ctc_b  (where the reference row is usable)  [+ reg / 2 * sum ||W||^2],

so autograd gives the parameter gradients.  The statistics (loss, expected, posterior, real, inactive) come from
tests/mwer_model.utterance on the same log-likelihoods, in caller order.

Rules restated here and broken one at a time by the ``mut_*`` switches (tests/test_brnn_mwer_model_cpu.py shows that each
changes a case):

* mut_rank_order        the per-utterance results come back in the engine's rank order (by length, descending, stable)
                        instead of caller order;
* mut_ref_in_posterior  the reference row takes part in the posterior, with error 0;
* mut_empty_skipped     a hypothesis without labels is not real;
* mut_ref_skip_kept     the lambda term of a reference whose CTC call skips is kept (its cost, +inf, enters the loss);
* mut_combine_sign      the MWER part of the gradient has the other sign.

`cases()` lists the minibatches tests/test_gpu_brnn_mwer.py runs; the CPU tests assert that none of them has a
pre-activation within 1e-5 of a kink (0, or max_act in the recurrent layer), where a float32 device and this model could
land on different sides."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import brnn as obrnn
from tests import mwer_model

MUTATIONS = ("mut_rank_order", "mut_ref_in_posterior", "mut_empty_skipped", "mut_ref_skip_kept", "mut_combine_sign")
MAX_ACT = 20.0


def to_torch(params):
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    return {"W": [t(w) for w in params["W"]], "b": [t(b) for b in params["b"]], "Wf": t(params["Wf"]), "Wb": t(params["Wb"])}


def forward(P, data, temporal_layer, max_act=MAX_ACT):
    """oracle.brnn.forward in torch ops.  P: to_torch(params); data (D, T).  Returns (logits (A, T), the smallest distance
    of a pre-activation from a kink)."""
    W, b = P["W"], P["b"]
    NL = len(W) - 1
    TL = temporal_layer if 0 < temporal_layer < NL else -1
    h = torch.as_tensor(np.asarray(data, dtype=np.float64))
    T = h.shape[1]
    kink = math.inf
    clip = lambda v: torch.clamp(v, min=0.0, max=max_act) if max_act is not None else torch.clamp(v, min=0.0)

    def near(v):
        d = float(v.detach().abs().min())
        if max_act is not None:
            d = min(d, float((v.detach() - max_act).abs().min()))
        return d

    for i in range(1, NL + 2):
        z = W[i - 1] @ h + b[i - 1]
        if i == TL:
            hF, hB = [None] * T, [None] * T
            pres = [z[:, 0], z[:, T - 1]]
            hF[0] = clip(z[:, 0])
            hB[T - 1] = clip(z[:, T - 1])
            for t in range(1, T):
                pf = z[:, t] + P["Wf"] @ hF[t - 1]
                hF[t] = clip(pf)
                u = T - 1 - t
                pb = z[:, u] + P["Wb"] @ hB[u + 1]
                hB[u] = clip(pb)
                pres += [pf, pb]
            kink = min(kink, min(near(v) for v in pres))
            h = torch.stack(hF, dim=1) + torch.stack(hB, dim=1)
        elif i <= NL:
            kink = min(kink, float(z.detach().abs().min()))
            h = torch.relu(z)
        else:
            h = z
    return h, kink


def ctc_cost(logits, labels):
    """(cost as a tensor with autograd and zero_infinity, whether the alignment is feasible) of one label row"""
    lp = logits.t().log_softmax(1).unsqueeze(1)         # [T, 1, A]
    T = lp.shape[0]
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    tg = torch.from_numpy(labels if labels.size else np.zeros(1, dtype=np.int64)).unsqueeze(0)
    il, tl = torch.tensor([T]), torch.tensor([labels.size])
    with torch.no_grad():
        plain = F.ctc_loss(lp, tg, il, tl, blank=0, reduction="none", zero_infinity=False)
    cost = F.ctc_loss(lp, tg, il, tl, blank=0, reduction="none", zero_infinity=True)[0]
    return cost, bool(torch.isfinite(plain[0]))


def step(params, data_list, hyps_list, errors_list, labels_list, temporal_layer, scale=1.0, subtract_mean=True,
         ctc_weight=0.0, reg=0.0, reg_in_grad=True, max_act=MAX_ACT, K=None, K_b=None, mut_rank_order=False,
         mut_ref_in_posterior=False, mut_empty_skipped=False, mut_ref_skip_kept=False, mut_combine_sign=False):
    """The whole step.  Returns a dict: loss, expected, ctc_cost [B]; inactive, ctc_skip bool [B]; posterior, coef
    float64 [B, K]; real bool [B, K]; grads {"W", "b", "Wf", "Wb"} float64 NumPy like oracle.brnn's; kink, the smallest
    distance of a pre-activation from a kink; loglik [B, K] (-inf where the CTC call is infeasible or was not made)."""
    P = to_torch(params)
    B = len(data_list)
    K = K or max([1] + [len(h) for h in hyps_list])
    K_b = [len(h) for h in hyps_list] if K_b is None else list(K_b)
    out = dict(loss=np.zeros(B), expected=np.zeros(B), ctc_cost=np.zeros(B), inactive=np.zeros(B, dtype=bool),
               ctc_skip=np.zeros(B, dtype=bool), posterior=np.zeros((B, K)), coef=np.zeros((B, K)),
               real=np.zeros((B, K), dtype=bool), loglik=np.full((B, K), -np.inf))
    total = torch.zeros((), dtype=torch.float64)
    kink = math.inf
    for b in range(B):
        logits, kk = forward(P, data_list[b], temporal_layer, max_act)
        kink = min(kink, kk)
        T = logits.shape[1]
        ll = [None] * K
        W = [float("nan")] * K
        for k in range(min(K_b[b], len(hyps_list[b]), K)):
            W[k] = float(errors_list[b][k])
            if not math.isfinite(W[k]):
                continue
            if mut_empty_skipped and len(hyps_list[b][k]) == 0:
                continue
            cost, ok = ctc_cost(logits, hyps_list[b][k])
            if ok:
                ll[k] = -cost
        lam_cost, lam_ok = None, False
        if ctc_weight > 0:
            lam_cost, lam_ok = ctc_cost(logits, labels_list[b])
            out["ctc_cost"][b] = float(lam_cost.detach()) if lam_ok else math.inf
            out["ctc_skip"][b] = not lam_ok
        llv = [float(v.detach()) if v is not None else -math.inf for v in ll]
        Wv = list(W)
        if mut_ref_in_posterior and lam_ok:
            ll, llv, Wv = ll + [-lam_cost], llv + [-float(lam_cost.detach())], Wv + [0.0]
        Kx = len(llv)
        u = mwer_model.utterance(llv, Wv, Kx if Kx > K else K_b[b], T, scale, subtract_mean)
        out["loglik"][b] = llv[:K]
        out["loss"][b] = u["loss"]
        out["expected"][b] = u["expected"]
        out["inactive"][b] = not u["active"]
        out["posterior"][b] = u["posterior"][:K]
        out["coef"][b] = u["coef"][:K]
        out["real"][b] = u["real"][:K]
        if u["active"]:
            real = list(u["real"])
            lt = torch.stack([ll[k] if real[k] else torch.zeros((), dtype=torch.float64) for k in range(Kx)])
            part = mwer_model.loss_from_ll(lt, Wv, real, scale, subtract_mean)
            total = total + (-part if mut_combine_sign else part)
        if ctc_weight > 0:
            if lam_ok:
                total = total + ctc_weight * lam_cost
                out["loss"][b] += ctc_weight * float(lam_cost.detach())
            elif mut_ref_skip_kept:
                out["loss"][b] += ctc_weight * math.inf
    if reg > 0 and reg_in_grad:
        mats = list(P["W"]) + ([P["Wf"], P["Wb"]] if P["Wf"] is not None else [])
        total = total + sum((reg / 2.0) * (m * m).sum() for m in mats)
    if total.requires_grad:
        total.backward()
    g = lambda t: None if t is None else (t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape)))
    out["grads"] = {"W": [g(w) for w in P["W"]], "b": [g(v) for v in P["b"]], "Wf": g(P["Wf"]), "Wb": g(P["Wb"])}
    out["kink"] = kink
    if mut_rank_order:
        order = sorted(range(B), key=lambda b: -np.asarray(data_list[b]).shape[1])
        for key in ("loss", "expected", "ctc_cost", "inactive", "ctc_skip", "posterior", "coef", "real", "loglik"):
            out[key] = out[key][order]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the minibatches of tests/test_gpu_brnn_mwer.py


class Case:
    def __init__(self, name, seed, A, T_b, K, D=10, H=16, NL=3, TL=2, K_b=None, scale=1.0, ctc_weight=0.0, reg=0.0,
                 subtract_mean=True, empty=(), equal=(), nan=(), long=(), ref_long=(), all_nan=False):
        """empty / nan / long: (b, k) pairs whose hypothesis is empty / has a NaN error / is longer than its frames;
        equal: (b, k, k2) -- hypothesis k2 is a copy of k; ref_long: utterances whose reference is longer than their
        frames (its CTC call skips)"""
        self.name, self.seed, self.A, self.T_b, self.K, self.D, self.H, self.NL, self.TL = name, seed, A, list(T_b), K, D, H, NL, TL
        self.scale, self.ctc_weight, self.reg, self.subtract_mean = scale, ctc_weight, reg, subtract_mean
        rs = np.random.RandomState(seed)
        self.params = obrnn.init_params(D, A, H, NL, TL, rng=rs)
        self.params["b"] = [0.1 * rs.randn(*b.shape) for b in self.params["b"]]
        B = len(T_b)
        self.data = [rs.randn(D, T) for T in T_b]
        self.K_b = list(K_b) if K_b is not None else [K] * B
        row = lambda T: rs.randint(1, A, size=rs.randint(1, max(2, min(5, T // 2 + 1)))).astype(np.int32)
        self.hyps = [[row(T_b[b]) for _ in range(self.K_b[b])] for b in range(B)]
        self.errors = [np.array([float(rs.randint(0, 6)) for _ in range(self.K_b[b])]) for b in range(B)]
        self.labels = [row(T_b[b]) for b in range(B)]
        for b, k in empty:
            self.hyps[b][k] = np.zeros(0, dtype=np.int32)
        for b, k, k2 in equal:
            self.hyps[b][k2] = self.hyps[b][k].copy()
        for b, k in nan:
            self.errors[b][k] = float("nan")
        for b, k in long:
            self.hyps[b][k] = rs.randint(1, A, size=T_b[b] + 2).astype(np.int32)
        for b in ref_long:
            self.labels[b] = rs.randint(1, A, size=T_b[b] + 1).astype(np.int32)
        if all_nan:
            self.errors = [np.full(len(e), np.nan) for e in self.errors]

    def host_stack(self):
        """the parameters in NNet.setParams' order"""
        st = [[w, b] for w, b in zip(self.params["W"], self.params["b"])]
        if self.params["Wf"] is not None:
            st += [[self.params["Wf"], None], [self.params["Wb"], None]]
        return st

    def model(self, **kw):
        args = dict(scale=self.scale, subtract_mean=self.subtract_mean, ctc_weight=self.ctc_weight, reg=self.reg, K=self.K,
                    K_b=self.K_b)
        args.update(kw)
        return step(self.params, self.data, self.hyps, self.errors, self.labels, self.TL, **args)


def cases():
    """name -> Case.  The seeds are chosen so that no pre-activation lies within 1e-5 of a kink (asserted on the CPU)."""
    cs = [
        Case("k1", 1, 5, [9], 1),
        Case("b3_k2", 2, 5, [7, 12, 9], 2),
        Case("ragged_empty_equal_lam", 3, 33, [7, 12, 9], 3, K_b=[3, 1, 2], ctc_weight=0.5, empty=[(0, 1)], equal=[(0, 0, 2)]),
        Case("a70_k8_nan_long_scale", 4, 70, [7, 12, 9], 8, scale=30.0, nan=[(1, 2)], long=[(0, 3), (2, 0)]),
        Case("a300_lam1", 5, 300, [10, 14], 3, H=32, ctc_weight=1.0),
        Case("k256", 6, 5, [14], 256),
        Case("one_frame", 7, 33, [8, 1, 6], 2),
        Case("all_inactive", 8, 5, [5, 6], 2, all_nan=True),
        Case("all_inactive_lam", 9, 5, [5, 6], 2, all_nan=True, ctc_weight=0.7),
        Case("ref_skips", 10, 33, [7, 12, 9], 2, ctc_weight=0.4, ref_long=[1]),
        Case("scale0", 11, 5, [7, 12, 9], 3, scale=0.0, subtract_mean=False),
        Case("tl0_reg", 12, 33, [9, 6], 3, TL=0, reg=0.01, ctc_weight=0.2),
        Case("uniform_lam", 13, 33, [7, 12, 9], 3, ctc_weight=0.3),
    ]
    return {c.name: c for c in cs}
