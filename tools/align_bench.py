"""CTC forced alignment throughput on synthetic batches with fixed seeds:

  (a) 256 utterances of T=1000, U=100, A=33 (the wave kernel, back-pointers on chip);
  (b) the long-utterance shape, T=8000, U=800, A=33, 8 and 128 utterances (the wide kernel,
      back-pointers in the workspace).

One JSON line per batch: milliseconds of the device call (hipEvents around sctc_ctc_align_batch,
everything already on the device) without and with SCTC_ALIGN_TOTAL; of the same call on a copy of
the batch whose last frame is all -inf, which runs the whole recursion and then has no path to
trace back (status 1), so the difference is the trace-back; of sctc_ctc_loss_batch on the same
batch (alpha, beta and the gradient: more arithmetic per cell); and of the NumPy restatement of
the contract (tests/align_model.py, vectorised over states) on the host, measured on a few
utterances and scaled to the batch.  The device results are checked against the restatement on
those utterances.

    python tools/align_bench.py [--reps 5] [--only a|b8|b128]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import _sctc  # noqa: E402
import ctc_fast  # noqa: E402
from tests import align_model  # noqa: E402


def event_ms(torch, run, reps):
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def bench(torch, L, name, B, T, U, A, reps, host_utts):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + B)
    logp = torch.log_softmax(2.0 * torch.randn(B * T, A, generator=g, device="cuda", dtype=torch.float32), dim=1)
    rs = np.random.RandomState(B + T)
    seqs = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
    labels = torch.from_numpy(np.concatenate(seqs)).cuda()
    Tb, Ub = np.full(B, T, np.int32), np.full(B, U, np.int32)
    fo, lo = (np.arange(B, dtype=np.int64) * T), (np.arange(B, dtype=np.int64) * U)
    fl = torch.empty(B * T, dtype=torch.int32, device="cuda")
    span = torch.empty(B * U * 2, dtype=torch.int32, device="cuda")
    scores = torch.empty(B * 2, dtype=torch.float64, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")

    def cfg_of(flags):
        return _sctc.AlignConfig(B, A, _sctc.F32, 0, A, flags, _sctc.i32(Tb), _sctc.i64(fo), _sctc.i32(Ub), _sctc.i64(lo))
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg_of(0)), ctypes.byref(nbytes)), "align")
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device="cuda")

    def align(src, flags):
        cfg = cfg_of(flags)

        def run():
            rc = L.sctc_ctc_align_batch(ctypes.byref(cfg), src.data_ptr(), labels.data_ptr(), fl.data_ptr(), span.data_ptr(),
                                        scores.data_ptr(), status.data_ptr(), ws.data_ptr() if nbytes.value else None,
                                        nbytes.value, _sctc.current_stream_ptr())
            _sctc.check(rc, "align")
        return run

    ms = event_ms(torch, align(logp, 0), reps)
    ms_total = event_ms(torch, align(logp, _sctc.ALIGN_TOTAL), reps)
    # check a few utterances against the restatement, and time it
    got_fl, got_sc, got_st = fl.cpu().numpy(), scores.cpu().numpy().reshape(B, 2), status.cpu().numpy()
    assert np.all(got_st == 0)
    host_s = []
    for b in range(host_utts):
        y = logp[b * T:(b + 1) * T].cpu().numpy().T
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            want = align_model.align(y, seqs[b], total=True)
        host_s.append(time.perf_counter() - t0)
        assert want.viterbi == got_sc[b, 0] and np.array_equal(want.frame_label, got_fl[b * T:(b + 1) * T])
        assert abs(want.total - got_sc[b, 1]) <= 1e-11 * abs(want.total)
    host_ms = float(np.median(host_s)) * 1e3 * B
    # the recursion alone: no path survives the last frame, nothing is traced back
    cut = logp.clone()
    cut.view(B, T, A)[:, T - 1, :] = float("-inf")
    ms_rec = event_ms(torch, align(cut, 0), reps)
    assert np.all(status.cpu().numpy() == 1)
    del cut
    # ctc_loss_batch on the same batch
    probs = torch.exp(logp)
    del logp
    grad = torch.empty_like(probs)
    lab_host = np.concatenate(seqs)
    bt = _sctc.CtcBatch(B, A, 0, _sctc.F32, A, _sctc.i32(Tb), _sctc.i32(Ub), _sctc.i64(fo), _sctc.i32(lab_host), _sctc.i64(lo),
                        ctypes.c_void_p(0))
    nb = L.sctc_ctc_workspace_bytes(ctypes.byref(bt))
    ws2 = torch.empty(nb, dtype=torch.uint8, device="cuda")
    cost = torch.empty(B, dtype=torch.float64, device="cuda")
    skip = torch.empty(B, dtype=torch.int32, device="cuda")

    def loss():
        _sctc.check(L.sctc_ctc_loss_batch(ctypes.byref(bt), probs.data_ptr(), grad.data_ptr(), cost.data_ptr(), skip.data_ptr(),
                                          ws2.data_ptr(), nb, _sctc.current_stream_ptr()), "ctc_loss")
    ms_loss = event_ms(torch, loss, reps)
    c = cost.cpu().numpy()
    loss_rel = float(np.max(np.abs(c + got_sc[:, 1]) / np.abs(c)))      # the loss kernels' cost against the float64 total
    plan = ctc_fast.align_plan(U)
    print(json.dumps({
        "batch": name, "B": B, "T": T, "U": U, "A": A, "path": plan["path"], "states_per_thread": plan["spl"],
        "workspace_bytes": nbytes.value, "align_ms": round(ms, 4), "align_total_ms": round(ms_total, 4),
        "recursion_only_ms": round(ms_rec, 4), "traceback_ms": round(ms - ms_rec, 4),
        "ctc_loss_ms": round(ms_loss, 4), "numpy_host_ms": round(host_ms, 1), "numpy_utts_measured": host_utts,
        "align_over_ctc_loss": round(ms / ms_loss, 3), "numpy_over_align": round(host_ms / ms, 1),
        "cells_per_s": round(B * T * (2 * U + 1) / ms * 1e3), "ctc_loss_cost_vs_total_rel": loss_rel}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("a", "b8", "b128"))
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    for name, B, T, U, host_utts in (("a", 256, 1000, 100, 4), ("b8", 8, 8000, 800, 1), ("b128", 128, 8000, 800, 1)):
        if a.only in (None, name):
            bench(torch, L, name, B, T, U, 33, a.reps, host_utts)


if __name__ == "__main__":
    main()
