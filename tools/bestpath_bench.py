"""Batched best-path decoding and device-side evaluation on seeded inputs:

  (a) 256 utterances of T = 1000 frames over A = 33 symbols, (b) 8 utterances of T = 8000: float64 (A, T)
      probability arrays whose arg-max path has runs of about three frames, every other run the blank.
      Timed: ``ctc_fast.decode_best_path_batch`` on the host arrays (upload, one launch, read-back); the kernel
      alone (hipEvents around ``sctc_ctc_bestpath_batch``, rows already on the device) with the row-to-lane
      mapping left to the library and forced either way (SCTC_BESTPATH_MAP); and the route this replaces on the
      same arrays, written out here: per utterance one upload, ``sctc_argmax_rows``, one read-back and the
      Python collapse of ``ctc_fast.collapse_best_path``.  The two routes must give the same labels.
  (c) a small network (D = 60, H = 128, 3 layers, temporal layer 2, A = 33; 64 utterances of T = 200):
      ``NNet.evaluate`` next to the host route -- ``forwardProbs`` per group, ``np.log``, the Python collapse and
      the host loop ``runDecode.edit_distance`` per utterance.

  (d) where the batched call's time goes on host arrays (packing, upload, the call on a device tensor), and the
      kernel under both mappings at A = 16 .. 300 (float32, 256 x 1000): the ground of the switch at A = 64.

One JSON line.    python tools/bestpath_bench.py [--reps 5]
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
from nnets import brnnet  # noqa: E402


def utterance(rs, T, A):
    """float64 (A, T) Fortran-ordered probabilities with a planted arg-max path of short runs"""
    path = []
    while len(path) < T:
        s = 0 if rs.rand() < 0.5 else int(rs.randint(1, A))
        path.extend([s] * int(rs.geometric(1.0 / 3.0)))
    path = np.array(path[:T])
    z = rs.rand(T, A)
    z[np.arange(T), path] += 4.0
    p = np.exp(z)
    p /= p.sum(axis=1, keepdims=True)
    return np.asfortranarray(p.T)


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def parent_route(torch, L, probs_list, blank=0):
    """what decode_best_path does, one utterance per call"""
    out = []
    for p in probs_list:
        A, T = p.shape
        dev = torch.from_numpy(p.T).cuda()
        best = torch.empty(T, dtype=torch.int32, device=dev.device)
        _sctc.check(L.sctc_argmax_rows(dev.data_ptr(), _sctc.F64, best.data_ptr(), T, A, A, _sctc.current_stream_ptr()),
                    "argmax_rows")
        out.append(ctc_fast.collapse_best_path(best.cpu().numpy(), blank))
    return out


def kernel_ms(torch, L, probs_list, reps, force=None, dtype=np.float64):
    """median hipEvent time of the C call alone, rows already on the device"""
    A = probs_list[0].shape[0]
    T_b = np.array([p.shape[1] for p in probs_list], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(T_b)[:-1]]).astype(np.int64)
    dev = torch.from_numpy(np.concatenate([np.ascontiguousarray(p.T, dtype=dtype) for p in probs_list])).cuda()
    cfg = _sctc.BestPathConfig(len(T_b), A, _sctc.F64 if dtype == np.float64 else _sctc.F32, 4,
                               (ctypes.c_int32 * 16)(0, 1, 2, 8), A, _sctc.i32(T_b), _sctc.i64(off))
    n = int(T_b.sum())
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    lens = torch.empty(len(T_b), dtype=torch.int32, device="cuda")
    spans = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    scores = torch.empty(len(T_b), dtype=torch.float64, device="cuda")

    def run():
        _sctc.check(L.sctc_ctc_bestpath_batch(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                              spans.data_ptr(), scores.data_ptr(), _sctc.current_stream_ptr()), "bestpath")
    if force:
        os.environ["SCTC_BESTPATH_MAP"] = force
    try:
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
    finally:
        os.environ.pop("SCTC_BESTPATH_MAP", None)
    return float(np.median(times)), dev.numel() * dev.element_size()


def call_parts(torch, probs_list, reps):
    """where the time of the batched call on host arrays goes: packing the list into one host block, the upload
    of that block, and the read-back of ids, lengths and spans with the split into per-utterance arrays"""
    pack = median_ms(lambda: np.concatenate([np.ascontiguousarray(p.T) for p in probs_list]), reps)
    host = np.concatenate([np.ascontiguousarray(p.T) for p in probs_list])

    def upload():
        torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
    up = median_ms(upload, reps)
    dev = torch.from_numpy(host).cuda()
    T_b = [p.shape[1] for p in probs_list]
    rest = median_ms(lambda: ctc_fast.decode_best_path_batch(dev, lengths=T_b), reps)
    return {"pack_ms": round(pack, 3), "upload_ms": round(up, 3), "device_tensor_call_ms": round(rest, 3),
            "megabytes": round(host.nbytes / 1e6, 1)}


def switch_sweep(torch, L, reps, B=256, T=1000):
    """both mappings on either side of the switch (float32 rows, the network's type)"""
    out = {}
    for A in (16, 33, 64, 65, 128, 300, 1024, 4096):
        rs = np.random.RandomState(A)
        n = B if A <= 300 else B * 300 // A        # the same bytes beyond A = 300
        probs = [utterance(rs, T, A).astype(np.float32) for _ in range(n)]
        lane, _ = kernel_ms(torch, L, probs, reps, "lane", np.float32)
        wave, _ = kernel_ms(torch, L, probs, reps, "wave", np.float32)
        out[str(A)] = {"B": n, "lane_ms": round(lane, 4), "wave_ms": round(wave, 4)}
    return out


def decode_shape(torch, L, B, T, A, reps, seed):
    rs = np.random.RandomState(seed)
    probs = [utterance(rs, T, A) for _ in range(B)]
    hyps, aligns = ctc_fast.decode_best_path_batch(probs)
    want = parent_route(torch, L, probs)
    for h, a, (wh, wa) in zip(hyps, aligns, want):
        assert h.tolist() == wh and a.tolist() == wa
    call = median_ms(lambda: ctc_fast.decode_best_path_batch(probs), reps)
    parent = median_ms(lambda: parent_route(torch, L, probs), max(1, reps // 2))
    k_auto, nbytes = kernel_ms(torch, L, probs, reps)
    k_lane, _ = kernel_ms(torch, L, probs, reps, "lane")
    k_wave, _ = kernel_ms(torch, L, probs, reps, "wave")
    return {"B": B, "T": T, "A": A, "batched_call_ms": round(call, 3), "parent_route_ms": round(parent, 3),
            "call_parts": call_parts(torch, probs, reps),
            "kernel_ms": round(k_auto, 4), "kernel_lane_ms": round(k_lane, 4), "kernel_wave_ms": round(k_wave, 4),
            "kernel_GBps": round(nbytes / k_auto / 1e6, 1), "labels": int(sum(len(h) for h in hyps))}


def evaluate_shape(torch, reps, B=64, T=200, D=60, H=128, A=33, maxUtts=16):
    rs = np.random.RandomState(99)
    np.random.seed(7)
    net = brnnet.NNet(D, A, H, 3, T, train=False, temporalLayer=2, maxUtts=maxUtts)
    net.initParams()
    data = [rs.randn(D, T).astype(np.float32) for _ in range(B)]
    refs = [rs.randint(1, A, size=30).astype(np.int32) for _ in range(B)]

    def host_route():
        stats, hyps = [], []
        with np.errstate(divide="ignore"):
            for g in range(0, B, maxUtts):
                for p, ref in zip(net.forwardProbs(data[g:g + maxUtts]), refs[g:g + maxUtts]):
                    logp = np.log(p)
                    hyp, _ = ctc_fast.collapse_best_path(np.argmax(logp, axis=0), 0)   # drops 0 and 1, 2, 8
                    stats.append(runDecode.edit_distance(list(ref), hyp))
                    hyps.append(hyp)
        return stats, hyps

    res = net.evaluate(data, refs, drop=(1, 2, 8))
    stats, hyps = host_route()
    assert res["stats"][:, 0].tolist() == [int(s) for s in stats]
    assert all(h.tolist() == w for h, w in zip(res["hyps"], hyps))
    dev_ms = median_ms(lambda: net.evaluate(data, refs, drop=(1, 2, 8)), reps)
    nocost_ms = median_ms(lambda: net.evaluate(data, refs, drop=(1, 2, 8), cost=False), reps)
    host_ms = median_ms(host_route, max(1, reps // 2))
    return {"B": B, "T": T, "evaluate_ms": round(dev_ms, 3), "evaluate_without_cost_ms": round(nocost_ms, 3),
            "host_route_ms": round(host_ms, 3), "errors": int(res["stats"][:, 0].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    out = {"a": decode_shape(torch, L, 256, 1000, 33, a.reps, 1234),
           "b": decode_shape(torch, L, 8, 8000, 33, a.reps, 5678),
           "evaluate": evaluate_shape(torch, a.reps), "switch_f32_256x1000": switch_sweep(torch, L, a.reps)}
    out["batched_faster_at_256x1000"] = bool(out["a"]["batched_call_ms"] < out["a"]["parent_route_ms"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
