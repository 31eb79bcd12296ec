"""Throughput of the prefix beam search with the recurrent character LM on the input
of tools/decode_bench.py: 256 utterances of T = 1000 frames, A = 35, float32 log-probabilities on the
device, beam 40 and 150, alpha 1.0, beta 0.5.  The LM: H = 1024, V = 40, seeded weights, Wh of spectral
norm 0.9.  One JSON line per beam: wall time of the decode call (hipEvents around
sctc_ctc_rnnbeam_decode_batch, descriptor upload included; median of --reps calls after a warm-up),
utterances/s, microseconds per frame, the new rows (recurrent steps) per frame and utterance and their
share of the beam, the share of the state copies, and the FLOP/s of the recurrent contraction
(2 * H * H per new entry) against the 157.3 TFLOP/s fp32 MFMA peak.

A step is made for every beam entry that is new in a frame.  The kernel does not report that number; it
is counted on the host by the search's restatement (tests/beam_model.py, fed with the device's own rows)
over the first --count-frames frames of --count-utts utterances (default 60 and 2).

The share of the state copies is measured, not derived: SCTC_RNNBEAM_STATE_COPIES=2 makes the kernel copy
the states of the carried entries twice per frame, which changes no result; the time this adds is the
time of one more copy, and its share of the ordinary call is reported.  It is a lower estimate: the repeated copy
reads and writes lines that the first one has just brought into L2.

Kernel times: run under ``rocprofv3 --kernel-trace --stats -- python tools/decode_rnn_bench.py``, in a
run of its own.

    python tools/decode_rnn_bench.py [--utts 256] [--frames 1000] [--reps 3] [--beams 40 150] [--hidden 1024]
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


def seeded_lm(V=40, H=1024, seed=0, rho=0.9):
    rs = np.random.RandomState(seed)
    toks = list(nn_lm.SPECIALS) + ["c%d" % i for i in range(V - 3)]
    Wx = (rs.randn(H, V) * 1.5 * np.sqrt(2.0)).astype(np.float32)
    Wh = rs.randn(H, H)
    Wh = (Wh * (rho / np.linalg.norm(Wh, 2))).astype(np.float32)
    bh = (0.1 * rs.randn(H)).astype(np.float32)
    Wo = (rs.randn(V, H) * 1.5 * np.sqrt(2.0 / H)).astype(np.float32)
    bo = (0.1 * rs.randn(V)).astype(np.float32)
    return nn_lm.RNNCharLM(toks, Wx, Wh, bh, Wo, bo)


def new_entries_per_frame(lp, beam, alpha, beta, dlm, frames):
    """mean number of beam entries per frame that were not in the previous frame's beam (each costs one
    recurrent step), from the search's restatement fed with the device's own rows"""
    from tests import beam_model
    cache = {}
    trace = []
    beam_model.decode(lp[:, :frames].astype(np.float64), beam, alpha, beta, lambda P: dlm.rows([P], cache=cache)[0],
                      trace=trace)
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
    ap.add_argument("--hidden", type=int, default=1024)
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
    lm = seeded_lm(H=a.hidden)
    sw = np.zeros(A, dtype=np.int32)
    sw[1:] = 3 + np.arange(A - 1)
    dlm = ctc_fast.DecodeRNNLM(lm, sw, A)
    flop_per_row = 2.0 * dlm.Hp * dlm.Hp
    Tb = np.full(B, T, dtype=np.int32)
    off = np.arange(B, dtype=np.int64) * T
    for beam in a.beams:
        cfg = _sctc.RNNBeamConfig(B, A, _sctc.F32, beam, 1, 0, A, _sctc.i32(Tb), _sctc.i64(off), alpha, beta,
                                  dlm.handle, _sctc.i32(sw))
        nbytes = L.sctc_ctc_rnnbeam_workspace_bytes(ctypes.byref(cfg))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ids = torch.empty(B * T, dtype=torch.int32, device="cuda")
        lens = torch.empty(B, dtype=torch.int32, device="cuda")
        scores = torch.empty(B, dtype=torch.float64, device="cuda")

        def run():
            rc = L.sctc_ctc_rnnbeam_decode_batch(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                                 scores.data_ptr(), ws.data_ptr(), nbytes, _sctc.current_stream_ptr())
            _sctc.check(rc, "decode")

        def timed(copies):
            """median seconds of the call with the carried states copied ``copies`` times per frame"""
            if copies == 1:
                os.environ.pop("SCTC_RNNBEAM_STATE_COPIES", None)
            else:
                os.environ["SCTC_RNNBEAM_STATE_COPIES"] = str(copies)
            try:
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
                return float(np.median(times)), float(max(times) - min(times))
            finally:
                os.environ.pop("SCTC_RNNBEAM_STATE_COPIES", None)
        t, spread = timed(1)
        score0, mean_len = float(scores[0]), float(lens.float().mean())
        t2, _ = timed(2)
        assert float(scores[0]) == score0, "the repeated copy changed a result"
        out = {"beam": beam, "lm": "rnn H=%d" % dlm.Hp, "utts": B, "frames": T, "A": A, "seconds": round(t, 4),
               "spread_s": round(spread, 4), "utts_per_s": round(B / t, 1), "us_per_frame": round(t * 1e6 / T, 2),
               "workspace_mb": round(nbytes / 2 ** 20, 1), "mean_len": mean_len, "score0": score0,
               "seconds_two_copies": round(t2, 4), "state_copy_share": round((t2 - t) / t, 4)}
        if a.count_utts > 0:
            nf = min(a.count_frames, T)
            per = float(np.mean([new_entries_per_frame(utts[b], beam, alpha, beta, dlm, nf)
                                 for b in range(min(a.count_utts, B))]))
            tiles = np.ceil(per / 32.0)
            out.update({"rows_per_frame": round(per, 2), "rows_share_of_beam": round(per / beam, 4),
                        "rec_gflop_per_s": round(per * flop_per_row * B * T / t / 1e9, 1),
                        "rec_share_of_mfma_peak": round(per * flop_per_row * B * T / t / PEAK, 5),
                        "tile_gflop_per_s": round(tiles * 32 * flop_per_row * B * T / t / 1e9, 1)})
        print(json.dumps(out), flush=True)
        del ws


if __name__ == "__main__":
    main()
