"""MBR selection over n-best lists on the device, on the input of tools/decode_bench.py: 256 utterances
of T = 1000 frames, A = 35, float32 log-probabilities on the device; the first pass is the n-gram search (5-gram fixture,
beam 40, alpha 1.0, beta 0.5) with nbest = 40, its output left on the device.

One JSON line with, each the median of --reps calls after a warm-up and with max - min as the spread (host clock ending in
a synchronise; nothing is read back):
  * ``mbr_<unit>_s`` / ``mbr_<unit>_conf_s``: ctc_fast.mbr_nbest(device=True) on the search's tensors, without and with
    confidences, for unit = char and word;
  * ``intern_s``: ctc_fast.intern_words alone on the same rows, one group per utterance;
  * ``old_route_est_s``: the route that existed before: the same K x K pairs of --old-utts utterances through
    ctc_fast.edit_distance_batch (host lists, 40 bytes of descriptor a pair) plus the risk loop in NumPy, scaled to all
    utterances -- an ESTIMATE, labelled so; in character unit;
  * ``edit_device_pairs_s``: the same unordered pairs, character unit, through ctc_fast.edit_distance_device on the
    search's tensors (40 bytes of descriptor a pair, built here once and not timed);
  * ``pairs``: the unordered pairs of real hypotheses, ``symbols`` and ``words``.
``--kernel-trace DIR``: instead of the above, three child runs of this tool under ``rocprofv3 --kernel-trace --stats``
(traces only, no counters), one per mode so that the two units do not share a kernel name's row: ``--profiled char``,
``--profiled word`` (both with confidences) and ``--profiled edit`` (the pairs through edit_distance_device).  A second
JSON line gives per mode the calls and the average microseconds of every nbest_* / intern_* / edit_distance kernel.

    python tools/mbr_bench.py [--utts 256] [--frames 1000] [--nbest 40] [--reps 5] [--old-utts 4] [--kernel-trace DIR]
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
import ctc_fast  # noqa: E402
from tools import decode_bench  # noqa: E402
from tools.rescore_bench import med  # noqa: E402


def old_route(rows, scores, scale):
    """K x K distances of one utterance through edit_distance_batch, then posteriors and risks in NumPy"""
    K = len(rows)
    a = [rows[k] for k in range(K) for j in range(K)]
    b = [rows[j] for k in range(K) for j in range(K)]
    D = ctc_fast.edit_distance_batch(a, b)[:, 0].reshape(K, K).astype(np.float64)
    real = np.isfinite(scores)
    w = np.where(real, np.exp(scale * (np.where(real, scores, 0.0) - scores[real].max())), 0.0)
    risk = (D * w[None, :]).sum(axis=1) / w.sum()
    return int(np.argmin(np.where(real, risk, np.inf)))


def pair_arrays(U, off, real, B, K):
    """(a_len, a_off, b_len, b_off) of the unordered pairs (k < j) of real hypotheses, utterance by utterance"""
    k, j = np.triu_indices(K, 1)
    a_len, a_off, b_len, b_off = [], [], [], []
    for b in range(B):
        keep = real[b, k] & real[b, j]
        ka, jb = b * K + k[keep], b * K + j[keep]
        a_len.append(U[ka]); a_off.append(off[ka]); b_len.append(U[jb]); b_off.append(off[jb])
    return tuple(np.concatenate(v) for v in (a_len, a_off, b_len, b_off))


def kernel_trace(a):
    """the three profiled child runs; the parent does not open the GPU"""
    out = {}
    for mode in ("char", "word", "edit"):
        d = os.path.join(a.kernel_trace, mode)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--utts", str(a.utts), "--frames", str(a.frames), "--nbest", str(a.nbest),
               "--reps", str(a.reps), "--profiled", mode]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    if any(t in r["Name"] for t in ("nbest_", "intern_", "edit_distance_kernel")):
                        name = re.search(r"(\w+_kernel(?:<[^>]*>)?)", r["Name"]).group(1)
                        rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                      "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        out[mode] = rows
    print(json.dumps({"kernels": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--nbest", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-utts", type=int, default=4, help="utterances timed on the old route (0: leave it out)")
    ap.add_argument("--kernel-trace", metavar="DIR", help="per-kernel times from three rocprofv3 child runs, written under DIR")
    ap.add_argument("--profiled", choices=("char", "word", "edit"), help="what a child run of --kernel-trace repeats")
    a = ap.parse_args()
    if a.kernel_trace:
        return kernel_trace(a)
    torch = _sctc.require_gpu()
    A, B, T, K = 35, a.utts, a.frames, a.nbest
    dev, ngram = decode_bench.load_input(torch, B, T, A)
    T_b = [T] * B
    sync = torch.cuda.synchronize
    trip = ctc_fast.decode_beam_batch(dev, T_b, beam=40, alpha=1.0, beta=0.5, lm=ngram, nbest=K, device=True)
    ids, lens, scores = trip
    sc = scores.reshape(B, K)
    U = lens.cpu().numpy().astype(np.int64)
    off = (K * (np.arange(B, dtype=np.int64) * T)[:, None] + np.arange(K, dtype=np.int64)[None, :] * T).reshape(-1)
    chars = {}
    with open(os.path.join(ROOT, "tests", "golden", "chars.txt")) as f:
        for line in f:
            tok, i = line.split()
            chars[tok] = int(i)
    space = chars["[space]"]
    out = {"utts": B, "frames": T, "nbest": K, "symbols": int(U.sum())}
    real = np.isfinite(sc.cpu().numpy())
    out["pairs"] = int((real.sum(axis=1) * (real.sum(axis=1) - 1) // 2).sum())
    pairs = pair_arrays(U, off, real, B, K)
    assert pairs[0].shape[0] == out["pairs"]

    def edit_pairs():
        return ctc_fast.edit_distance_device(ids, pairs[0], pairs[1], ids, pairs[2], pairs[3])
    if a.profiled:
        for _ in range(a.reps):
            if a.profiled == "edit":
                edit_pairs()
            else:
                ctc_fast.mbr_nbest(trip, sc, unit=a.profiled, scale=1.0, space=space, A=A, confidences=True, device=True,
                                   lengths=T_b)
        sync()
        return
    s, spread = med(edit_pairs, a.reps, sync)
    out["edit_device_pairs_s"], out["edit_device_pairs_spread_s"] = round(s, 6), round(spread, 6)
    d_old = edit_pairs()[:, 0].cpu().numpy()
    d_new = ctc_fast.mbr_nbest(trip, sc, unit="char", A=A, distances=True, device=True, lengths=T_b)["dist"].cpu().numpy()
    kk, jj = np.triu_indices(K, 1)
    out["edit_device_same_distances"] = bool((d_new[:, kk, jj][real[:, kk] & real[:, jj]] == d_old).all())
    for unit in ("char", "word"):
        for conf in (False, True):
            s, spread = med(lambda: ctc_fast.mbr_nbest(trip, sc, unit=unit, scale=1.0, space=space, A=A, confidences=conf,
                                                       device=True, lengths=T_b), a.reps, sync)
            name = "mbr_%s%s" % (unit, "_conf" if conf else "")
            out[name + "_s"], out[name + "_spread_s"] = round(s, 6), round(spread, 6)
    s, spread = med(lambda: ctc_fast.intern_words((ids, U, off), np.arange(B + 1) * K, space, A=A, device=True), a.reps, sync)
    out["intern_s"], out["intern_spread_s"] = round(s, 6), round(spread, 6)
    out["words"] = int(ctc_fast.intern_words((ids, U, off), np.arange(B + 1) * K, space, A=A, device=True)[1].sum().item())
    res = ctc_fast.mbr_nbest(trip, sc, unit="word", scale=1.0, space=space, A=A, device=True, lengths=T_b)
    out["changed_1best_word"] = int((res["best"] != 0).sum().item())
    if a.old_utts:
        n = min(a.old_utts, B)
        h_ids, h_sc = ids.cpu().numpy(), sc.cpu().numpy()
        lists = [[h_ids[off[b * K + k]:off[b * K + k] + U[b * K + k]] for k in range(K)] for b in range(n)]
        old_route(lists[0], h_sc[0], 1.0)
        sync()
        t0 = time.perf_counter()
        old_best = [old_route(lists[b], h_sc[b], 1.0) for b in range(n)]
        sync()
        dt = time.perf_counter() - t0
        out["old_route_utts"] = n
        out["old_route_s"] = round(dt, 4)
        out["old_route_est_s"] = round(dt * B / n, 3)
        new_best = ctc_fast.mbr_nbest(trip, sc, unit="char", scale=1.0, A=A, device=True, lengths=T_b)["best"].cpu().numpy()
        out["old_route_same_choice"] = int((np.array(old_best) == new_best[:n]).sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
