"""Throughput of the prefix beam search with the neural character LM on the input
of tools/decode_bench.py: 256 utterances of T = 1000 frames, A = 35, float32 log-probabilities on the
device, beam 40 and 150, alpha 1.0, beta 0.5.  The LM: K = 19, two hidden layers of 1024, V = 40,
seeded weights.  One JSON line per beam: wall time of the decode call (hipEvents around
sctc_ctc_nnbeam_decode_batch, descriptor upload included; median of --reps calls after a warm-up),
utterances/s, microseconds per frame, the LM rows evaluated per frame and utterance and their share
of the beam, and the FLOP/s of the row contractions (the matrix-core layers, 2 * in * out per row)
against the 157.3 TFLOP/s fp32 MFMA peak.

A row is evaluated for every beam entry that is new in a frame.  The kernel does not report that
number; it is counted on the host by the search's restatement (tests/beam_model.py, fed with the
device's own rows) over the first --count-frames frames of --count-utts utterances (default 60 and 2).

Kernel times: run under ``rocprofv3 --kernel-trace --stats -- python tools/decode_nn_bench.py``, in a
run of its own.

    python tools/decode_nn_bench.py [--utts 256] [--frames 1000] [--reps 3] [--beams 40 150]
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
import nn_lm  # noqa: E402

PEAK = 157.3e12


def posteriors(rs, A, T):
    """the generator of tools/decode_bench.py"""
    x = 1.5 * rs.randn(A, T)
    t = 0
    while t < T:
        s = rs.randint(1, A) if rs.rand() < 0.6 else 0
        r = rs.randint(1, 4)
        x[s, t:t + r] += 4.0
        t += r
    m = x.max(axis=0, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))).astype(np.float32)


def seeded_lm(V=40, K=19, hidden=(1024, 1024), seed=0):
    rs = np.random.RandomState(seed)
    toks = list(nn_lm.SPECIALS) + ["c%d" % i for i in range(V - 3)]
    widths = [K * V] + list(hidden) + [V]
    ws, bs = [], []
    for l in range(len(widths) - 1):
        fan = K if l == 0 else widths[l]
        ws.append((rs.randn(widths[l + 1], widths[l]) * 1.5 * np.sqrt(2.0 / fan)).astype(np.float32))
        bs.append((0.1 * rs.randn(widths[l + 1])).astype(np.float32))
    return nn_lm.NNCharLM(toks, K, ws, bs)


def new_entries_per_frame(lp, beam, alpha, beta, dlm, frames):
    """mean number of beam entries per frame that were not in the previous frame's beam (each costs one
    LM row), from the search's restatement fed with the device's own rows"""
    sys.path.insert(0, ROOT)
    from tests import beam_model
    cache = {}

    def row(P):
        if P not in cache:
            cache[P] = dlm.rows([P])[0]
        return cache[P]
    trace = []
    beam_model.decode(lp[:, :frames].astype(np.float64), beam, alpha, beta, row, trace=trace)
    prev, new = {()}, 0
    for fr in trace:
        cur = {P for P, _ in fr["beam"]}
        new += len(cur - prev)
        prev = cur
    return new / float(len(trace))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beams", type=int, nargs="+", default=[40, 150])
    ap.add_argument("--count-utts", type=int, default=2)
    ap.add_argument("--count-frames", type=int, default=60)
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    A, B, T = 35, a.utts, a.frames
    alpha, beta = 1.0, 0.5
    rs = np.random.RandomState(0)
    utts = [posteriors(rs, A, T) for _ in range(B)]
    dev = torch.from_numpy(np.concatenate([u.T for u in utts], axis=0)).cuda()
    lm = seeded_lm()
    sw = np.zeros(A, dtype=np.int32)
    sw[1:] = 3 + np.arange(A - 1)
    dlm = ctc_fast.DecodeNNLM(lm, sw, A)
    widths = lm.padded()[0]
    flop_per_row = sum(2.0 * widths[l] * widths[l + 1] for l in range(1, len(widths) - 1))
    Tb = np.full(B, T, dtype=np.int32)
    off = np.arange(B, dtype=np.int64) * T
    for beam in a.beams:
        cfg = _sctc.NNBeamConfig(B, A, _sctc.F32, beam, 1, 0, A, _sctc.i32(Tb), _sctc.i64(off), alpha, beta,
                                 dlm.handle, _sctc.i32(sw))
        nbytes = L.sctc_ctc_nnbeam_workspace_bytes(ctypes.byref(cfg))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ids = torch.empty(B * T, dtype=torch.int32, device="cuda")
        lens = torch.empty(B, dtype=torch.int32, device="cuda")
        scores = torch.empty(B, dtype=torch.float64, device="cuda")

        def run():
            rc = L.sctc_ctc_nnbeam_decode_batch(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                                scores.data_ptr(), ws.data_ptr(), nbytes, _sctc.current_stream_ptr())
            _sctc.check(rc, "decode")
        run()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
        t = float(np.median(times))
        out = {"beam": beam, "lm": "nn K=%d %s" % (lm.context, "x".join(str(w) for w in widths[1:-1])),
               "utts": B, "frames": T, "A": A, "seconds": round(t, 4), "utts_per_s": round(B / t, 1),
               "us_per_frame": round(t * 1e6 / T, 2), "workspace_mb": round(nbytes / 2 ** 20, 1),
               "mean_len": float(lens.float().mean()), "score0": float(scores[0])}
        if a.count_utts > 0:
            nf = min(a.count_frames, T)
            per = float(np.mean([new_entries_per_frame(utts[b], beam, alpha, beta, dlm, nf)
                                 for b in range(min(a.count_utts, B))]))
            tiles = np.ceil(per / 32.0)
            out.update({"rows_per_frame": round(per, 2), "rows_share_of_beam": round(per / beam, 4),
                        "row_gflop_per_s": round(per * flop_per_row * B * T / t / 1e9, 1),
                        "row_share_of_mfma_peak": round(per * flop_per_row * B * T / t / PEAK, 5),
                        "tile_gflop_per_s": round(tiles * 32 * flop_per_row * B * T / t / 1e9, 1)})
        print(json.dumps(out), flush=True)
        del ws


if __name__ == "__main__":
    main()
