"""N-best rescoring on the device against the host route, on the input of tools/decode_bench.py:
256 utterances of T = 1000 frames, A = 35, float32 log-probabilities on the device.  The first pass is the n-gram
search (5-gram fixture, beam 40, alpha 1.0, beta 0.5) with nbest = 40, its output left on the device; the second pass
re-ranks the 40-best of every utterance under the h1024 recurrent LM of tools/decode_rnn_bench.py, under the
feed-forward LM of tools/decode_nn_bench.py, and under the 5-gram itself.

One JSON line per LM with, each the median of --reps calls after a warm-up and with max - min as the spread:
  * ``device_s``: ctc_fast.rescore_nbest on the search's device tensors (one align launch, one LM-score call, one rank
    launch; the read-back of the lengths and the result included), and ``lm_score_s``: the LM-score call alone
    (hipEvents around sctc_lm_score_batch);
  * ``host_s``: the existing host route, ``align_batch(total=True)`` + ``lm_sentence_scores``, and ``device_same_s``: the
    device route on the same input.  The host route builds every prefix of every hypothesis as a Python tuple and makes
    one launch per prefix depth, so it is timed on the first --host-utts utterances only (default 2: 80 hypotheses);
    ``host_full_estimate_s`` scales that to the whole input by the number of LM terms;
  * the sums of the two routes on that input are compared for equal bits (``sums_equal``).
With --first-pass the first-pass neural searches (beam 40, the calls of decode_rnn_bench.py / decode_nn_bench.py) are
timed on the same posteriors, for context.  Kernel times: run under ``rocprofv3 --kernel-trace --stats -- python
tools/rescore_bench.py --host-utts 0``, in a run of its own.

    python tools/rescore_bench.py [--utts 256] [--frames 1000] [--nbest 40] [--reps 3] [--host-utts 2] [--first-pass]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import _sctc  # noqa: E402
import ctc_fast  # noqa: E402
from tools import decode_bench, decode_nn_bench, decode_rnn_bench  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--nbest", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-utts", type=int, default=2)
    ap.add_argument("--first-pass", action="store_true")
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    A, B, T, K = 35, a.utts, a.frames, a.nbest
    alpha, beta = 1.0, 0.5
    dev, ngram = decode_bench.load_input(torch, B, T, A)
    sw = np.zeros(A, dtype=np.int32)
    sw[1:] = 3 + np.arange(A - 1)
    lms = {"rnn h1024": ctc_fast.DecodeRNNLM(decode_rnn_bench.seeded_lm(), sw, A),
           "nn 2x1024 K=19": ctc_fast.DecodeNNLM(decode_nn_bench.seeded_lm(), sw, A),
           "5-gram": ngram}
    T_b = [T] * B
    sync = torch.cuda.synchronize
    t_first, _ = med(lambda: ctc_fast.decode_beam_batch(dev, T_b, beam=40, alpha=alpha, beta=beta, lm=ngram, nbest=K,
                                                        device=True), 1, sync)
    ids, lens, scores = ctc_fast.decode_beam_batch(dev, T_b, beam=40, alpha=alpha, beta=beta, lm=ngram, nbest=K, device=True)
    U = lens.cpu().numpy().astype(np.int64)
    off = (K * (np.arange(B, dtype=np.int64) * T)[:, None] + np.arange(K, dtype=np.int64)[None, :] * T).reshape(-1)
    n_terms = int(U.sum())
    hb = min(a.host_utts, B)
    sub = dev[:hb * T]
    for name, lm in lms.items():
        device_s, device_spread = med(lambda: ctc_fast.rescore_nbest(dev, (ids, lens, scores), lengths=T_b, lm=lm,
                                                                     alpha=alpha, beta=beta), a.reps, sync)
        order, _ = ctc_fast.rescore_nbest(dev, (ids, lens, scores), lengths=T_b, lm=lm, alpha=alpha, beta=beta)
        ev = []

        def lm_only():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctc_fast.lm_score_batch((ids, U, off), lm, device=True)
            e1.record()
            ev.append((e0, e1))
        lm_only()
        sync()
        del ev[:]
        for _ in range(a.reps):
            lm_only()
        sync()
        lm_times = [e0.elapsed_time(e1) / 1e3 for e0, e1 in ev]
        out = {"lm": name, "utts": B, "frames": T, "nbest": K, "lm_terms": n_terms, "first_pass_ngram_s": round(t_first, 4),
               "device_s": round(device_s, 5), "device_spread_s": round(device_spread, 5),
               "lm_score_s": round(float(np.median(lm_times)), 5),
               "lm_score_spread_s": round(max(lm_times) - min(lm_times), 5),
               "changed_1best": int((order[:, 0] != 0).sum())}
        if hb > 0:
            h_ids = ids.cpu().numpy()
            flat = [h_ids[off[p]:off[p] + U[p]].copy() for p in range(hb * K)]
            rows = torch.cat([sub[b * T:(b + 1) * T] for b in range(hb) for _ in range(K)])
            h_len = [T] * (hb * K)
            host_sums = []

            def host():
                ctc_fast.align_batch(rows, flat, lengths=h_len, total=True)
                host_sums[:] = [ctc_fast.lm_sentence_scores(flat, lm)]
            host_s, host_spread = med(host, a.reps, sync)
            same_s, same_spread = med(lambda: ctc_fast.rescore_nbest(sub, (ids[:hb * K * T], lens[:hb * K], scores[:hb * K]),
                                                                     lengths=T_b[:hb], lm=lm, alpha=alpha, beta=beta),
                                      a.reps, sync)
            dsum = ctc_fast.lm_score_batch((ids, U[:hb * K], off[:hb * K]), lm)
            sub_terms = int(U[:hb * K].sum())
            out.update({"host_utts": hb, "host_lm_terms": sub_terms, "host_s": round(host_s, 4),
                        "host_spread_s": round(host_spread, 4), "device_same_s": round(same_s, 5),
                        "device_same_spread_s": round(same_spread, 5), "host_over_device": round(host_s / same_s, 1),
                        "host_full_estimate_s": round(host_s * n_terms / max(sub_terms, 1), 1),
                        "sums_equal": bool(np.array_equal(dsum, host_sums[0]))})
        print(json.dumps(out), flush=True)
    if a.first_pass:
        for name, lm in list(lms.items())[:2]:
            t, spread = med(lambda: ctc_fast.decode_beam_batch(dev, T_b, beam=40, alpha=alpha, beta=beta, lm=lm, device=True),
                            a.reps, sync)
            print(json.dumps({"first_pass": name, "beam": 40, "utts": B, "frames": T, "seconds": round(t, 4),
                              "spread_s": round(spread, 4)}), flush=True)


if __name__ == "__main__":
    main()
