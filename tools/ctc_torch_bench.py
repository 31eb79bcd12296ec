"""Forward plus backward of ctc_torch.ctc_loss on seeded inputs, at T = 1000, C = 33, U = 100 -- the
headline's CTC shape -- with N = 32 and N = 256 utterances of full length, next to

  (a) ``ctc_fast.ctc_loss_batch`` on probabilities that are already packed on the device: the CTC kernels alone, so
      new - (a) is what the prologue, the epilogue and the autograd plumbing cost;
  (b) ``torch.nn.functional.ctc_loss`` on the device plus its backward under
      ``torch.backends.cudnn.flags(enabled=False)``: PyTorch's native kernels, not a vendor library.  Its input is the
      log_softmax computed beforehand (a leaf), like the input of the logits=False run.

Also timed alone: the prologue kernel (both modes) and the epilogue kernel, with the bytes they move.  Method: every
variant is warmed up, then timed ``--reps`` times with device events around ``--iters`` back-to-back calls; the median
per call is reported.  The variants alternate inside one process.  The losses of the three routes are compared first.

One JSON line.    timeout 600 python tools/ctc_torch_bench.py [--reps 7] [--iters 10] [--dtype float32]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import _sctc  # noqa: E402
import ctc_fast  # noqa: E402
import ctc_torch  # noqa: E402


def event_ms(torch, fn, reps, iters):
    """median milliseconds per call of fn, device events around `iters` calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def shape(torch, T, N, C, U, dtype, reps, iters):
    import torch.nn.functional as F
    rs = np.random.RandomState(1000 + N)
    tdt = torch.float64 if dtype == "float64" else torch.float32
    logits = torch.from_numpy(rs.randn(T, N, C)).to(tdt).cuda()
    logp = logits.log_softmax(2)
    seqs = [rs.randint(1, C, size=U).astype(np.int32) for _ in range(N)]
    targets = torch.from_numpy(np.stack(seqs).astype(np.int64))
    targets_dev = targets.cuda()
    il, tl = [T] * N, [U] * N
    il_t, tl_t = torch.tensor(il), torch.tensor(tl)
    # (a): utterance n owns rows n * T .. of the packed [N * T][C] probabilities
    packed = logits.softmax(2).transpose(0, 1).contiguous().reshape(N * T, C)

    x_logits = logits.clone().requires_grad_()
    x_logp = logp.clone().requires_grad_()

    def new(x, is_logits):
        x.grad = None
        ctc_torch.ctc_loss(x, targets, il, tl, reduction="sum", logits=is_logits).backward()

    def route_a():
        ctc_fast.ctc_loss_batch(packed, seqs, lengths=il)

    def route_b():
        x_logp.grad = None
        with torch.backends.cudnn.flags(enabled=False):
            F.ctc_loss(x_logp, targets_dev, il_t, tl_t, reduction="sum").backward()

    # the same numbers first
    with torch.no_grad():
        mine = ctc_torch.ctc_loss(logits, targets, il, tl, reduction="none", logits=True).double().cpu()
        mine_lp = ctc_torch.ctc_loss(logp, targets, il, tl, reduction="none").double().cpu()
        with torch.backends.cudnn.flags(enabled=False):
            native = F.ctc_loss(logp, targets_dev, il_t, tl_t, reduction="none").double().cpu()
    cost_a = ctc_fast.ctc_loss_batch(packed, seqs, lengths=il)[0].cpu()
    rel = lambda a, b: float(((a - b).abs() / b.abs()).max())

    # the two new kernels alone
    L = _sctc.lib()
    T_dev = torch.tensor(il, dtype=torch.int32).cuda()
    probs = torch.empty((T * N, C), dtype=tdt, device="cuda")
    out = torch.empty_like(logits)
    cost = torch.zeros(N, dtype=torch.float64, device="cuda")
    skip = torch.zeros(N, dtype=torch.int32, device="cuda")
    scale = torch.ones(N, dtype=torch.float64, device="cuda")
    st = logits.stride()
    cfgs = {m: _sctc.TncConfig(T, N, C, _sctc.F64 if dtype == "float64" else _sctc.F32, m, 0, *st)
            for m in (_sctc.TNC_LOG_PROBS, _sctc.TNC_LOGITS)}

    def prologue(mode, src):
        _sctc.check(L.sctc_ctc_tnc_probs(ctypes.byref(cfgs[mode]), src.data_ptr(), T_dev.data_ptr(), probs.data_ptr(),
                                         _sctc.current_stream_ptr()), "tnc_probs")

    def epilogue():
        _sctc.check(L.sctc_ctc_tnc_grad(ctypes.byref(cfgs[0]), probs.data_ptr(), T_dev.data_ptr(), cost.data_ptr(),
                                        skip.data_ptr(), scale.data_ptr(), out.data_ptr(), _sctc.current_stream_ptr()),
                    "tnc_grad")

    variants = {
        "new_logits_ms": lambda: new(x_logits, True),
        "new_logprobs_ms": lambda: new(x_logp, False),
        "a_ctc_loss_batch_ms": route_a,
        "b_torch_native_ms": route_b,
        "prologue_softmax_ms": lambda: prologue(_sctc.TNC_LOGITS, logits),
        "prologue_exp_ms": lambda: prologue(_sctc.TNC_LOG_PROBS, logp),
        "epilogue_ms": epilogue,
    }
    res = {"T": T, "N": N, "C": C, "U": U, "dtype": dtype,
           "loss_rel_diff_new_vs_a": rel(mine, cost_a), "loss_rel_diff_new_vs_b": rel(mine, native),
           "loss_rel_diff_logprobs_vs_b": rel(mine_lp, native)}
    spread = {}
    for name, fn in variants.items():
        med, lo, hi = event_ms(torch, fn, reps, iters)
        res[name] = round(med, 4)
        spread[name] = [round(lo, 4), round(hi, 4)]
    res["min_max_ms"] = spread
    nbytes = 2 * T * N * C * logits.element_size()          # each of the two kernels reads and writes T * N * C once
    res["prologue_epilogue_megabytes_each"] = round(nbytes / 1e6, 2)
    res["prologue_softmax_GBps"] = round(nbytes / res["prologue_softmax_ms"] / 1e6, 1)
    res["epilogue_GBps"] = round(nbytes / res["epilogue_ms"] / 1e6, 1)
    res["prologue_epilogue_share_of_new_logits"] = round((res["prologue_softmax_ms"] + res["epilogue_ms"]) / res["new_logits_ms"], 3)
    res["new_logits_over_a"] = round(res["new_logits_ms"] / res["a_ctc_loss_batch_ms"], 3)
    res["new_logprobs_over_b"] = round(res["new_logprobs_ms"] / res["b_torch_native_ms"], 3)
    res["new_logits_over_b"] = round(res["new_logits_ms"] / res["b_torch_native_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    out = {"reps": a.reps, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "shapes": [shape(torch, 1000, N, 33, 100, a.dtype, a.reps, a.iters) for N in (32, 256)]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
