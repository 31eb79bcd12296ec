"""Batched edit distance throughput on synthetic pairs with fixed seeds:

  (a) 256 references of 120..200 symbols over 34 symbols, each with a hypothesis that is the
      reference with about 10 % random edits: counts and paths (SCTC_EDIT_OPS);
  (b) the same 256 references against 40 hypotheses each, 10 240 pairs: distance only.

One JSON line: kernel milliseconds (hipEvents around sctc_edit_distance_batch, sequences
already on the device) and whole-call milliseconds (ctc_fast.edit_distance_batch on host
lists: conversion, upload, launch, read-back) for both sets, pairs/s and cells/s of the
kernel, the milliseconds of the host loop runDecode.edit_distance over the pairs of (a), and
-- in the same process, on the input of tools/decode_bench.py -- the milliseconds of the
decode call at beam 40 without an LM, which is what scoring is compared with.

    python tools/edit_bench.py [--reps 5]
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
import runDecode  # noqa: E402
from tools import decode_bench  # noqa: E402


def edited(rs, ref, rate=0.10, A=34):
    hyp = list(ref)
    for _ in range(max(1, int(round(rate * len(ref))))):
        kind, pos = rs.randint(3), int(rs.randint(0, len(hyp)))
        if kind == 0:
            hyp.insert(pos, int(rs.randint(1, A + 1)))
        elif kind == 1 and len(hyp) > 1:
            del hyp[pos]
        else:
            hyp[pos] = int(rs.randint(1, A + 1))
    return np.array(hyp, dtype=np.int32)


def kernel_ms(torch, L, a_seqs, b_seqs, a_index, ops, reps):
    """median hipEvent time of the C call alone, everything already on the device"""
    P = len(b_seqs)
    la = np.array([len(s) for s in a_seqs], dtype=np.int64)
    lb = np.array([len(s) for s in b_seqs], dtype=np.int64)
    sa = np.concatenate([[0], np.cumsum(la)])[:-1]
    a_len = np.ascontiguousarray(la[a_index], dtype=np.int32)
    a_off = np.ascontiguousarray(sa[a_index], dtype=np.int64)
    b_len = np.ascontiguousarray(lb, dtype=np.int32)
    b_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lb)])[:-1], dtype=np.int64)
    cfg = _sctc.EditConfig(P, _sctc.EDIT_OPS if ops else 0, _sctc.i32(a_len), _sctc.i64(a_off), _sctc.i32(b_len),
                           _sctc.i64(b_off))
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), "edit")
    a_dev = torch.from_numpy(np.concatenate(a_seqs)).cuda()
    b_dev = torch.from_numpy(np.concatenate(b_seqs)).cuda()
    stats = torch.empty(P * 5, dtype=torch.int32, device="cuda")
    n_ops = int((a_len.astype(np.int64) + b_len).sum()) if ops else 0
    codes = torch.empty(max(1, n_ops), dtype=torch.int8, device="cuda")
    lens = torch.empty(P, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device="cuda")

    def run():
        rc = L.sctc_edit_distance_batch(ctypes.byref(cfg), a_dev.data_ptr(), b_dev.data_ptr(), stats.data_ptr(),
                                        codes.data_ptr() if ops else None, lens.data_ptr() if ops else None,
                                        ws.data_ptr() if nbytes.value else None, nbytes.value,
                                        _sctc.current_stream_ptr())
        _sctc.check(rc, "edit")
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
    cells = float((a_len.astype(np.int64) * b_len).sum())
    return float(np.median(times)), cells, nbytes.value


def call_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def decode_ms(torch, L, reps, B=256, T=1000, A=35, beam=40):
    """tools/decode_bench.py's own measurement, on its input, at beam 40 without an LM"""
    dev, lm = decode_bench.load_input(torch, B, T, A)
    return decode_bench.measure(torch, L, dev, lm, B, T, A, beam, False, reps)[0] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    rs = np.random.RandomState(1234)
    refs = [rs.randint(1, 35, size=int(rs.randint(120, 201))).astype(np.int32) for _ in range(256)]
    hyp_a = [edited(rs, r) for r in refs]
    rs = np.random.RandomState(5678)
    hyp_b = [edited(rs, refs[i], rate=0.05 + 0.01 * k) for i in range(256) for k in range(40)]
    idx_a = np.arange(256)
    idx_b = np.repeat(np.arange(256), 40)

    ka, cells_a, ws_a = kernel_ms(torch, L, refs, hyp_a, idx_a, True, a.reps)
    kb, cells_b, _ = kernel_ms(torch, L, refs, hyp_b, idx_b, False, a.reps)
    ca = call_ms(lambda: ctc_fast.edit_distance_batch(refs, hyp_a, ops=True), a.reps)
    cb = call_ms(lambda: ctc_fast.edit_distance_batch(refs, hyp_b, a_index=idx_b), a.reps)
    stats = ctc_fast.edit_distance_batch(refs, hyp_a)
    t0 = time.perf_counter()
    host = [runDecode.edit_distance(list(r), list(h)) for r, h in zip(refs, hyp_a)]
    host_ms = (time.perf_counter() - t0) * 1e3
    assert host == stats[:, 0].tolist()
    dec = decode_ms(torch, L, a.reps)
    print(json.dumps({
        "a_pairs": 256, "a_kernel_ms": round(ka, 4), "a_call_ms": round(ca, 3), "a_workspace_bytes": ws_a,
        "a_pairs_per_s": round(256 / ka * 1e3), "a_cells_per_s": round(cells_a / ka * 1e3),
        "b_pairs": len(hyp_b), "b_kernel_ms": round(kb, 4), "b_call_ms": round(cb, 3),
        "b_pairs_per_s": round(len(hyp_b) / kb * 1e3), "b_cells_per_s": round(cells_b / kb * 1e3),
        "host_loop_a_ms": round(host_ms, 1), "decode_beam40_nolm_ms": round(dec, 3),
        "a_call_below_decode": bool(ca < dec), "mean_dist_a": float(stats[:, 0].mean())}), flush=True)


if __name__ == "__main__":
    main()
