"""MWER training over n-best lists on the device: forward plus backward of ctc_torch.mwer_loss at
T = 1000 frames, C = 33 symbols, hypotheses of about 100 labels, N = 32 utterances, K in {4, 8}, float32 activations
(``logits=True``), next to ctc_torch.ctc_loss on N * K utterances of the same shapes -- the same CTC work without the
K-fold prologue and the combine pass, so it is the floor.

One JSON line with, per K (host clock around forward + backward, ending in a synchronise; the two losses are timed
alternately, twice each: the lower of the two medians of --reps calls after a warm-up, the larger max - min as spread):
  * ``mwer_k<K>_s``: mwer_loss and its backward;
  * ``ctc_floor_k<K>_s``: ctc_loss on [T, N * K, C] with the same label rows, and its backward;
  * ``ratio_k<K>``: the first over the second;
  * ``bytes_probs_k<K>`` / ``bytes_combine_k<K>``: the bytes the prologue and the combine kernel move, from the shapes
    (prologue: the input once, the K-fold probabilities once; combine: one rank's probabilities and the K-fold gradient
    rows read, one [T * N][C] result written).
``--kernel-trace DIR``: instead, one child run of this tool per K under ``rocprofv3 --kernel-trace --stats`` (traces only,
no counters; the program after ``--``).  A second JSON line gives per K the calls and the average microseconds of the
three ctc_mwer_* kernels and, from the bytes above, their achieved bytes/s.

    python tools/mwer_bench.py [--utts 32] [--frames 1000] [--labels 100] [--reps 7] [--kernel-trace DIR]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import _sctc  # noqa: E402

C = 33
KS = (4, 8)


def med(fn, reps, sync):
    fn()
    sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(max(times) - min(times))


def traffic(T, N, K, itemsize=4):
    """bytes moved by the prologue and by the combine kernel, every frame live and every rank real"""
    rows = T * N * C * itemsize
    return rows + K * rows, rows + K * rows + rows


def kernel_trace(a):
    """one profiled child run per K; the parent does not open the GPU"""
    out = {}
    for K in KS:
        d = os.path.join(a.kernel_trace, "k%d" % K)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--utts", str(a.utts), "--frames", str(a.frames), "--labels", str(a.labels),
               "--reps", str(a.reps), "--profiled", str(K)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        b_probs, b_comb = traffic(a.frames, a.utts, K)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    if "ctc_mwer_" in r["Name"]:
                        name = re.search(r"(ctc_mwer_\w+_kernel)", r["Name"]).group(1)
                        avg = float(r["AverageNs"])
                        row = {"calls": int(r["Calls"]), "avg_us": round(avg / 1e3, 2),
                               "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
                        if "probs" in name:
                            row["bytes_per_s"] = round(b_probs / (avg * 1e-9), -6)
                        if "combine" in name:
                            row["bytes_per_s"] = round(b_comb / (avg * 1e-9), -6)
                        rows[name] = row
        out["k%d" % K] = rows
    print(json.dumps({"kernels": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-trace", metavar="DIR", help="per-kernel times from one rocprofv3 child run per K, written under DIR")
    ap.add_argument("--profiled", type=int, choices=KS, help="what a child run of --kernel-trace repeats")
    a = ap.parse_args()
    if a.kernel_trace:
        return kernel_trace(a)
    torch = _sctc.require_gpu()
    import ctc_torch
    T, N, U = a.frames, a.utts, a.labels
    sync = torch.cuda.synchronize
    rs = np.random.RandomState(0)
    out = {"utts": N, "frames": T, "labels": U, "alphabet": C, "dtype": "float32"}
    for K in ((a.profiled,) if a.profiled else KS):
        lens = rs.randint(U - 10, U + 11, size=(N, K))
        S = int(lens.max())
        hyps = torch.from_numpy(rs.randint(1, C, size=(N, K, S)).astype(np.int64))
        lengths = torch.from_numpy(lens.astype(np.int64))
        errors = torch.from_numpy(rs.randint(0, 12, size=(N, K)).astype(np.float64))
        x = torch.from_numpy(rs.randn(T, N, C).astype(np.float32)).cuda().requires_grad_()
        il = [T] * N
        # the floor: the same label rows as N * K utterances of a plain CTC loss, utterance n * K + k <- (n, k)
        xk = x.detach().repeat_interleave(K, dim=1).contiguous().requires_grad_()
        targets, tl, ilk = hyps.reshape(N * K, S), lengths.reshape(N * K), [T] * (N * K)

        def mwer():
            x.grad = None
            ctc_torch.mwer_loss(x, hyps, lengths, errors, il, logits=True).backward()

        def floor():
            xk.grad = None
            ctc_torch.ctc_loss(xk, targets, ilk, tl, reduction="sum", logits=True).backward()

        if a.profiled:
            for _ in range(a.reps):
                mwer()
            sync()
            return
        # alternating, so that a drift of the box hits both
        m1, sp1 = med(mwer, a.reps, sync)
        f1, fs1 = med(floor, a.reps, sync)
        m2, sp2 = med(mwer, a.reps, sync)
        f2, fs2 = med(floor, a.reps, sync)
        m, f = min(m1, m2), min(f1, f2)
        out["mwer_k%d_s" % K], out["mwer_k%d_spread_s" % K] = round(m, 6), round(max(sp1, sp2), 6)
        out["ctc_floor_k%d_s" % K], out["ctc_floor_k%d_spread_s" % K] = round(f, 6), round(max(fs1, fs2), 6)
        out["ratio_k%d" % K] = round(m / f, 3)
        out["bytes_probs_k%d" % K], out["bytes_combine_k%d" % K] = traffic(T, N, K)
        stats = ctc_torch.mwer_loss(x, hyps, lengths, errors, il, logits=True, return_stats=True)[1]
        out["real_k%d" % K] = int(stats["real"].sum().item())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
