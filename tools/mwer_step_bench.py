"""The MWER step of the native model on the device: NNet.mwerCostAndGradBatch at the headline shape
(T = 1000 frames, 5 x 1824 units, temporal layer 3, 33 symbols, minibatch 32, fp32, hypotheses of about 100 labels,
K in {4, 8}, ctc_weight 0 and 0.3), next to NNet.costAndGradBatch on the same minibatch (the CTC step) and to K such
calls (what the fused step replaces: the forward and backward passes paid K times).

One JSON line with, per K and ctc_weight (host clock around a call, ending in a synchronise; the versions alternate in
one process after a warm-up; the median of --reps calls and max - min as the spread):
  * ``ctc_step_s``: costAndGradBatch on the references;
  * ``mwer_k<K>_lam<0|1>_s``: mwerCostAndGradBatch;
  * ``k_calls_k<K>_s``: K calls of costAndGradBatch, hypothesis k as every utterance's label row;
  * ``ratio_step_*``: the MWER step over the CTC step; ``ratio_calls_*``: the K calls over the MWER step;
  * ``bytes_spread_k<K>`` / ``bytes_combine_k<K>``: the bytes the two row kernels move, from the shapes.
``--kernel-trace DIR``: instead, one child run of this tool per K under ``rocprofv3 --kernel-trace --stats`` (traces only,
no counters; the program after ``--``).  A second JSON line gives per K the calls and the average microseconds of the
three brnn_mwer_* kernels and, from the bytes above, their achieved bytes/s.

    python tools/mwer_step_bench.py [--utts 32] [--frames 1000] [--labels 100] [--layer 1824] [--reps 5] [--kernel-trace DIR]
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

A = 33
D = 41 * 15
KS = (4, 8)
LAM = 0.3


def traffic(N, K, lam, itemsize=4):
    """bytes moved by the spread and the combine kernel over N frames, every rank real; S = K (+ 1 with a CTC term)"""
    S = K + (1 if lam else 0)
    row = N * A * itemsize
    return row + S * row, row + S * row + row


def kernel_trace(a):
    """one profiled child run per K; the parent does not open the GPU"""
    out = {}
    for K in KS:
        d = os.path.join(a.kernel_trace, "k%d" % K)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--utts", str(a.utts), "--frames", str(a.frames), "--labels", str(a.labels),
               "--layer", str(a.layer), "--reps", str(a.reps), "--profiled", str(K)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        b_spread, b_comb = traffic(a.frames * a.utts, K, LAM)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    m = re.search(r"(brnn_mwer_(?:spread|empty|combine)_kernel)", r["Name"])
                    if not m:
                        continue
                    avg = float(r["AverageNs"])
                    row = {"calls": int(r["Calls"]), "avg_us": round(avg / 1e3, 2),
                           "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
                    if "spread" in m.group(1):
                        row["bytes_per_s"] = round(b_spread / (avg * 1e-9), -6)
                    if "combine" in m.group(1):
                        row["bytes_per_s"] = round(b_comb / (avg * 1e-9), -6)
                    rows[m.group(1)] = row
        out["k%d" % K] = rows
    print(json.dumps({"kernels": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=100)
    ap.add_argument("--layer", type=int, default=1824)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-trace", metavar="DIR", help="per-kernel times from one rocprofv3 child run per K, written under DIR")
    ap.add_argument("--profiled", type=int, choices=KS, help="what a child run of --kernel-trace repeats")
    a = ap.parse_args()
    if a.kernel_trace:
        return kernel_trace(a)
    torch = _sctc.require_gpu()
    from nnets import brnnet
    T, B, U = a.frames, a.utts, a.labels
    sync = torch.cuda.synchronize
    rs = np.random.RandomState(0)
    np.random.seed(0)
    net = brnnet.NNet(D, A, a.layer, 5, T, temporalLayer=3, maxUtts=B)
    net.initParams()
    feats = torch.from_numpy(rs.randn(B * T, D).astype(np.float32)).cuda()
    T_b = [T] * B
    refs = [rs.randint(1, A, size=rs.randint(U - 10, U + 11)).astype(np.int32) for _ in range(B)]
    out = {"utts": B, "frames": T, "labels": U, "alphabet": A, "layer": a.layer, "dtype": "float32", "ctc_weight": LAM}

    def timed(fns):
        """the versions alternate; per version the median and the spread of --reps calls after one warm-up each"""
        for fn in fns.values():
            fn()
        sync()
        times = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                sync()
                times[k].append(time.perf_counter() - t0)
        return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in times.items()}

    for K in ((a.profiled,) if a.profiled else KS):
        hyps = [[rs.randint(1, A, size=rs.randint(U - 10, U + 11)).astype(np.int32) for _ in range(K)] for _ in range(B)]
        errs = [rs.randint(0, 12, size=K).astype(np.float64) for _ in range(B)]
        mwer = lambda lam: net.mwerCostAndGradBatch(None, hyps, errs, labels_list=refs if lam else None, ctc_weight=lam,
                                                    feats_dev=feats, T_b=T_b)
        if a.profiled:
            for _ in range(a.reps):
                mwer(LAM)
            sync()
            return
        fns = {"ctc_step": lambda: net.costAndGradBatch(None, refs, feats_dev=feats, T_b=T_b),
               "mwer_lam0": lambda: mwer(0.0), "mwer_lam1": lambda: mwer(LAM),
               "k_calls": lambda: [net.costAndGradBatch(None, [h[k] for h in hyps], feats_dev=feats, T_b=T_b)
                                   for k in range(K)]}
        r = timed(fns)
        out["ctc_step_s"], out["ctc_step_spread_s"] = r["ctc_step"]
        for lam in (0, 1):
            out["mwer_k%d_lam%d_s" % (K, lam)], out["mwer_k%d_lam%d_spread_s" % (K, lam)] = r["mwer_lam%d" % lam]
            out["ratio_step_k%d_lam%d" % (K, lam)] = round(r["mwer_lam%d" % lam][0] / r["ctc_step"][0], 4)
        out["k_calls_k%d_s" % K], out["k_calls_k%d_spread_s" % K] = r["k_calls"]
        out["ratio_calls_k%d" % K] = round(r["k_calls"][0] / r["mwer_lam0"][0], 4)
        out["bytes_spread_k%d" % K], out["bytes_combine_k%d" % K] = traffic(B * T, K, 0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
