"""Prefix beam search decoder throughput: 256 utterances of T = 1000 frames,
A = 35, float32 log-probabilities on the device, beam 40 and 150, without an LM and with the
5-gram character LM fixture.  One JSON line per configuration: wall time of the decode call
(hipEvents around sctc_ctc_beam_decode_batch, descriptor upload included), utterances/s and
microseconds per frame (all utterances advance together).  Kernel times: run under
``rocprofv3 --kernel-trace --stats -- python tools/decode_bench.py``.

    python tools/decode_bench.py [--utts 256] [--frames 1000] [--reps 3]
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
import arpa_lm  # noqa: E402
import ctc_fast  # noqa: E402


def posteriors(rs, A, T):
    x = 1.5 * rs.randn(A, T)
    t = 0
    while t < T:
        s = rs.randint(1, A) if rs.rand() < 0.6 else 0
        r = rs.randint(1, 4)
        x[s, t:t + r] += 4.0
        t += r
    m = x.max(axis=0, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))).astype(np.float32)


def load_input(torch, B, T, A=35):
    """the bench's posteriors on the device and the 5-gram character LM fixture"""
    rs = np.random.RandomState(0)
    rows = np.concatenate([posteriors(rs, A, T).T for _ in range(B)], axis=0)
    dev = torch.from_numpy(rows).cuda()
    golden = os.path.join(ROOT, "tests", "golden")
    chars = {}
    with open(os.path.join(golden, "chars.txt")) as f:
        for line in f:
            tok, i = line.split()
            chars[int(i)] = tok
    lm = ctc_fast.DecodeLM(arpa_lm.ArpaLM(os.path.join(golden, "lm_char_5g.arpa")), chars, A)
    return dev, lm


def measure(torch, L, dev, lm, B, T, A, beam, with_lm, reps):
    """median seconds of the decode call (hipEvents), its workspace bytes, lengths and scores"""
    Tb = np.full(B, T, dtype=np.int32)
    off = np.arange(B, dtype=np.int64) * T
    sw = np.ascontiguousarray(lm.sym_words, dtype=np.int32)
    cfg = _sctc.BeamConfig(B, A, _sctc.F32, beam, 1, 0, A, _sctc.i32(Tb), _sctc.i64(off), 1.0, 0.5,
                           lm.handle if with_lm else None, _sctc.i32(sw))
    nbytes = L.sctc_ctc_beam_workspace_bytes(ctypes.byref(cfg))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ids = torch.empty(B * T, dtype=torch.int32, device="cuda")
    lens = torch.empty(B, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, dtype=torch.float64, device="cuda")

    def run():
        rc = L.sctc_ctc_beam_decode_batch(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                          scores.data_ptr(), ws.data_ptr(), nbytes, _sctc.current_stream_ptr())
        _sctc.check(rc, "decode")
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(times)), nbytes, lens, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    A, B, T = 35, a.utts, a.frames
    dev, lm = load_input(torch, B, T, A)
    for beam in (40, 150):
        for with_lm in (False, True):
            t, nbytes, lens, scores = measure(torch, L, dev, lm, B, T, A, beam, with_lm, a.reps)
            print(json.dumps({"beam": beam, "lm": "5-gram" if with_lm else None, "utts": B, "frames": T, "A": A,
                              "seconds": round(t, 4), "utts_per_s": round(B / t, 1),
                              "us_per_frame": round(t * 1e6 / T, 2), "workspace_mb": round(nbytes / 2 ** 20, 1),
                              "mean_len": float(lens.float().mean()), "score0": float(scores[0])}), flush=True)


if __name__ == "__main__":
    main()
