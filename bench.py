#!/usr/bin/env python3
"""Headline benchmark: audio frames/sec of one full costAndGrad (BRNN forward + softmax/CTC
+ BRNN backward, weight gradients resident on the device; data-parallel: after the RCCL
all-reduce) at the WSJ shape of BASELINE.json configs[2]:
T=1000, |alphabet|=33, 5x1824 BRNN (temporalLayer 3, inputDim 483), U=100, minibatch 32 per GPU.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N>1: either under a launcher -- python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
     --gpus N ... -- or plain: without RANK / WORLD_SIZE in the environment the script starts that launcher itself)

Prints ONE JSON line on rank 0.  Synthetic features/labels (SURVEY 8(d) generators), reference
weight init, fp32 arithmetic like the reference's cudamat path.  Weak scaling: every GPU
processes its own 32 utterances; the only exchange is the sum of the weight gradients.

The metric is SURVEY 8(d)'s: the features of a step start in PINNED HOST memory; their H2D copy
runs on a copy stream into one of two device buffers, so the upload of step k+1 overlaps the
compute of step k (all K uploads sit inside the timed region).  `value` = frames / wall time of
exactly K such steps (barrier + synchronize on both sides, max over ranks), `ms_per_step` = that
wall time / K.  A plain run does only that: set-up, W warm-up steps, the K timed steps, the line.
--dump-outputs DIR writes what the last timed step returned to its caller (dump_outputs); the
inputs are seeded, so two builds can be compared output for output.

--full adds everything else, outside the timed region unless said otherwise: the CPU baseline
(before the HIP runtime starts), phase timers during the K timed steps (the roofline legs), the
same K steps with the features already RESIDENT in HBM (side field `hbm_resident`: what the
kernels alone do; round 3 reported that as `value`, rounds 1-2 and 4 the pinned-host pipeline),
one utterance's cost checked against the float64 oracle (a mismatch fails the run), the side
measurements and other configurations (--no-side / --no-cpu-baseline leave parts out), and for
N>1 the exchange's timing and the N = 1 step time it is compared with.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

# the host driver only supports dmabuf IPC: RCCL (and any CUDA-tensor sharing across processes) needs
# this before the HIP runtime starts
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "stanford-ctc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# cfg-3 of SURVEY 8(d)
CFG = dict(D=483, A=33, H=1824, NL=5, TL=3, T=1000, U=100, B=32)
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: dense f32 matrix peak
PEAK_HBM_GBPS = 8000.0
PEAK_F16_MFMA_TFLOPS = 2500.0   # dense f16/bf16 MFMA peak
PHASES = ["fwd_gemm", "fwd_rec", "ctc", "bwd_gemm", "bwd_rec", "other"]


_CPU_CTX = None      # (cfg, params): set by the parent before forking -- the workers share the weight pages


def _cpu_utt(job):
    """one cfg-3-shaped utterance (T frames) through the oracle; worker of both CPU legs.  The
    weights come from the parent (fork, copy-on-write: every process reads the SAME physical
    pages, like the threads of one trainer would), the utterance is the worker's own."""
    seed, threads, T = job
    cfg, params = _CPU_CTX
    from oracle import brnn as obrnn
    try:
        from threadpoolctl import threadpool_limits
        ctx = threadpool_limits(limits=threads)
    except Exception:
        import contextlib
        ctx = contextlib.nullcontext()
    rs = np.random.RandomState(seed)
    with ctx, np.errstate(all="ignore"):
        data = rs.randn(cfg["D"], T)
        labels = rs.randint(1, cfg["A"], size=max(1, T // 10)).astype(np.int32)
        t0 = time.time()
        obrnn.cost_and_grad(params, data, labels, cfg["TL"], max_act=20.0)
        return t0, time.time()


def cpu_baseline(cfg, budget_s=75.0):
    """The oracle (NumPy float64 BRNN restatement of rnnetcpu.py + C restatement of
    ctc_fast.pyx) timed on the host cores for a bounded sample of the same workload, two legs
    (SURVEY 8(d)):
      single thread  = stand-in for the reference's GIL-bound ctc_loss + one-core NumPy: one
                       whole utterance of T frames;
      all cores      = the reference's only parallelism is independent jobs (sgd.py:70-95 is one
                       utterance at a time, cluster/utils.py launches processes): P processes x
                       t BLAS threads, one utterance each, SWEPT from one process per core down
                       to a few fat ones; the best split is the reported figure and `cores` is
                       what it used.  Sample utterances are T/4 frames long (the cost is linear in
                       T, the matrices and the memory behaviour are those of the full shape) so
                       that the whole sweep stays within ~1 minute of host time."""
    global _CPU_CTX
    import multiprocessing as mp
    from oracle import brnn as obrnn
    ncpu = os.cpu_count() or 1
    _CPU_CTX = (cfg, obrnn.init_params(cfg["D"], cfg["A"], cfg["H"], cfg["NL"], cfg["TL"],
                                       rng=np.random.RandomState(10)))
    try:
        a, b = _cpu_utt((0, 1, cfg["T"]))
        t1 = b - a
        single = {"value": cfg["T"] / t1, "unit": "frames/s", "cores": 1,
                  "sample": "1 utterance of T=%d (cfg-3 shape), %.1f s, one thread" % (cfg["T"], t1)}
        Ts = max(50, cfg["T"] // 4)
        # from a few fat processes to one per core.  The recurrence is 4000 matrix-vector products
        # over 2 x 26.6 MB of float64 weights per utterance: memory-bound, so the curve peaks early
        # (measured on the 256-core GPU host: 16x2 2223, 128x1 1386, 256x1 1275 frames/s) -- the sweep
        # stops after two splits in a row that fall short of the best so far, or when its budget is up
        splits = []
        for procs, threads in ((8, 8), (16, 2), (16, 4), (32, 2), (32, 4), (ncpu // 4, 1), (ncpu // 4, 2),
                               (ncpu // 2, 1), (ncpu // 2, 2), (ncpu, 1)):
            procs = max(1, min(procs, ncpu // max(1, threads)))
            if (procs, threads) not in splits:
                splits.append((procs, threads))
        tried = []
        t_sweep = time.time()
        worse = 0
        for procs, threads in splits:
            if tried and (time.time() - t_sweep > budget_s or worse >= 2):
                break
            with mp.get_context("fork").Pool(procs) as pool:
                spans = pool.map(_cpu_utt, [(100 + i, threads, Ts) for i in range(procs)], chunksize=1)
            wall = max(e for _, e in spans) - min(b for b, _ in spans)
            rate = procs * Ts / wall
            worse = worse + 1 if (tried and rate < max(tried)[0]) else 0
            tried.append((rate, procs, threads, wall, float(np.mean([e - b for b, e in spans])), Ts))
        # the far end of the curve is measured in every run, whatever the early stop decided: ONE PROCESS
        # PER CORE (shorter utterances, T/16, so that ~250 memory-bound processes still finish in seconds)
        every_core = None
        if not any(p == ncpu and t == 1 for _, p, t, _, _, _ in tried):
            Tc = max(50, cfg["T"] // 16)
            with mp.get_context("fork").Pool(ncpu) as pool:
                spans = pool.map(_cpu_utt, [(300 + i, 1, Tc) for i in range(ncpu)], chunksize=1)
            wall = max(e for _, e in spans) - min(b for b, _ in spans)
            every_core = (ncpu * Tc / wall, Tc, wall)
            tried.append((every_core[0], ncpu, 1, wall, float(np.mean([e - b for b, e in spans])), Tc))
    finally:
        _CPU_CTX = None
    best = max(tried)
    return {"value": best[0], "unit": "frames/s", "cores": best[1] * best[2],
            "kind": "port, extrapolated from T=%d utterances (the like-for-like T=%d figure is single_thread: %.0f frames/s on one core)"
                    % (best[5], cfg["T"], single["value"]),
            "host_cores": ncpu,
            "sample": "best of a sweep over processes x BLAS threads on the %d host cores: %d utterances "
                      "of T=%d (cfg-3 shape, a fraction of the headline length) in %d processes x %d "
                      "threads sharing one copy of the weights, %.1f s wall, %.1f s mean per utterance; "
                      "NumPy f64 BRNN oracle + C CTC oracle; memory-bound on the host, run-to-run and "
                      "box-to-box spread +-15 %% (1.9-2.5 k frames/s over rounds 2-3); sweep: %s"
                      % (ncpu, best[1], best[5], best[1], best[2], best[3], best[4],
                         ", ".join("%dx%d -> %.0f frames/s" % (p, t, v) for v, p, t, _, _, _ in tried)) +
                      ("" if every_core is None else
                       " (the last point, one process per core, always measured, on utterances of T=%d: "
                       "%.1f s wall)" % (every_core[1], every_core[2])),
            "every_core": None if every_core is None else
                          {"value": every_core[0], "unit": "frames/s", "cores": ncpu, "T": every_core[1]},
            "single_thread": single}


def oracle_cost_check(cfg, net, feats_one, labels_one, cost_gpu):
    """one utterance of the benchmarked minibatch through the float64 oracle's forward pass +
    CTC (outside the timed region); the run FAILS if the GPU cost is off by more than 1e-4 rel"""
    from oracle import brnn as obrnn
    from oracle import ctc as octc
    NL, TL = cfg["NL"], cfg["TL"]
    params = {"W": [], "b": [], "Wf": None, "Wb": None}
    for i in range(NL + 1):
        params["W"].append(net.stack[i][0].copy_to_host().astype(np.float64))
        params["b"].append(net.stack[i][1].copy_to_host().astype(np.float64))
    params["Wf"] = net.stack[NL + 1][0].copy_to_host().astype(np.float64)
    params["Wb"] = net.stack[NL + 2][0].copy_to_host().astype(np.float64)
    with np.errstate(all="ignore"):
        logits, _ = obrnn.forward(params, feats_one.astype(np.float64).T, TL, 20.0)
        c_ref, _, skip = octc.ctc_loss(np.asfortranarray(obrnn.softmax_cols(logits)),
                                       np.ascontiguousarray(labels_one, dtype=np.int32), 0)
    err = abs(cost_gpu - c_ref) / abs(c_ref)
    if skip or not np.isfinite(cost_gpu) or err > 1e-4:
        raise SystemExit("bench.py: GPU cost %.6f != oracle %.6f (rel %.2e): parity broken, no "
                         "number reported" % (cost_gpu, c_ref, err))
    return {"utterance": 0, "gpu": float(cost_gpu), "oracle": float(c_ref), "rel_err": float(err)}


DUMP_SAMPLE = 1 << 20       # entries kept of a gradient matrix larger than this


def dump_outputs(d, net, cost, skip):
    """--dump-outputs: what the last timed step returned to its caller (costAndGradBatch: cost, grad stack, skip), one
    DIR/<name>.npy each -- cost (float64 [B]), skip (float32 0 / 1 [B]), grad_W<i> / grad_b<i> for the NL + 1
    feed-forward layers and grad_Wf / grad_Wb of the temporal layer (float32).  The whole gradient is 84 MB at the
    headline shape: a matrix of more than DUMP_SAMPLE entries is written as DUMP_SAMPLE of them, at row-major positions
    drawn from a fixed seed and sorted (the same positions in every run), 28 MB in all."""
    os.makedirs(d, exist_ok=True)
    arrays = {"cost": np.asarray(cost, dtype=np.float64), "skip": np.asarray(skip, dtype=np.float32)}
    NL = net.numLayers
    for i, (w, b) in enumerate(net.grad):
        if i <= NL:
            arrays["grad_W%d" % (i + 1)] = w.copy_to_host()
            arrays["grad_b%d" % (i + 1)] = b.copy_to_host()
        else:                                       # the temporal pair's bias is a shared dummy, not a gradient
            arrays["grad_W%s" % ("f" if i == NL + 1 else "b")] = w.copy_to_host()
    for name, a in arrays.items():
        if a.size > DUMP_SAMPLE:
            idx = np.sort(np.random.RandomState(7).choice(a.size, DUMP_SAMPLE, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(d, name + ".npy"), a)


def self_launch(n):
    """`python bench.py --gpus N` without a launcher around it (no RANK / WORLD_SIZE in the environment): re-run
    this very command line under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N` on 127.0.0.1 and a
    free port -- one rank per GPU over RCCL, exactly what the driver's documented N>1 line starts.  The children
    inherit stdout / stderr (rank 0 prints the one JSON line); their exit status is ours."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")      # torch.distributed.run would set 1 (and say so on stderr)
    print("bench.py: --gpus %d without a launcher, starting %s" % (n, " ".join(cmd[1:9])), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def csrc_hash():
    """hash of the kernel sources: a PMC summary is only read back when it was measured on
    these sources (tools/profile_bench.sh stores the same hash)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "stanford-ctc_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "stanford-ctc_amd", "csrc", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also the CPU baseline, roofline, oracle cost check, side measurements and other "
                         "configurations (a plain run times the headline steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-side", action="store_true",
                    help="--full without the PCIe-inclusive, ragged and other side measurements (profiling runs)")
    ap.add_argument("--batch", type=int, default=CFG["B"], help="utterances per GPU")
    ap.add_argument("--n1-ms", type=float, default=None,
                    help="--full, N > 1: the single-GPU step time (ms, HBM-resident features) to compare with; default: "
                         "measured in this run, every rank stepping alone on its own GPU before the data-parallel steps")
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: launch the N ranks ourselves (VERDICT r04 missing #4)
        raise SystemExit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # the CPU legs fork worker processes: run them before the HIP runtime exists in this process
    cpu_base = cpu_baseline(dict(CFG)) if (args.full and world == 1 and not args.no_cpu_baseline) else None
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    # SCTC_BENCH_BACKEND=gloo lets several ranks share one GPU (plumbing test of the N>1 path
    # on a 1-GPU box); the real run uses nccl (= RCCL over xGMI), one rank per GPU
    backend = os.environ.get("SCTC_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local % torch.cuda.device_count())
    # SCTC_BENCH_FORCE_DP=1: a single rank takes the data-parallel path anyway (process group,
    # per-layer all-reduces queued behind the gradient events, barrier + MAX over ranks) -- the
    # 1-GPU rehearsal of the driver's N>1 launch with the real backend (RCCL)
    force_dp = world == 1 and os.environ.get("SCTC_BENCH_FORCE_DP", "0") == "1"
    if force_dp:
        os.environ["SCTC_DIST_SINGLE_RANK"] = "1"
        os.environ.setdefault("MASTER_PORT", "29571")
    if world > 1 or force_dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        kw = {}
        if backend == "nccl":                      # bind the communicator to this rank's GPU up front
            kw["device_id"] = torch.device("cuda", torch.cuda.current_device())
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    assert world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus

    import _sctc
    from nnets import brnnet
    import dist_sgd

    cfg = dict(CFG)
    cfg["B"] = args.batch
    D, A, H, NL, TL, T, U, B = (cfg[k] for k in ("D", "A", "H", "NL", "TL", "T", "U", "B"))
    np.random.seed(0)                       # identical initial weights on every rank
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B, gemm="f32")   # the reference's fp32 arithmetic
    net.initParams()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + rank)
    feats = torch.randn(B * T, D, device="cuda", generator=gen)     # reference copy, resident in HBM
    rs = np.random.RandomState(100 + rank)
    labels = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
    Ts = [T] * B
    dp = dist_sgd.DataParallel(net) if (world > 1 or force_dp) else None
    if dp is not None and world > 1 and backend != "gloo":
        # one rank per PHYSICAL GPU (the ranks exchanged PCI bus ids in DataParallel.__init__): two RCCL
        # ranks on one device would be refused by RCCL later with a less readable message
        assert len(set(dp.device_ids)) == world and not dp.shared_device, \
            "bench.py --gpus %d: ranks share a GPU (%s); SCTC_BENCH_BACKEND=gloo rehearses on fewer devices" \
            % (world, dp.device_ids)
    # "features already in pinned host memory -> H2D -> ..."
    host_feats = torch.empty(B * T, D, dtype=torch.float32).pin_memory()
    host_feats.copy_(feats)
    dev_bufs = [torch.empty_like(feats), torch.empty_like(feats)]
    copy_stream = torch.cuda.Stream()
    ev_ready = [torch.cuda.Event(), torch.cuda.Event()]
    ev_free = [torch.cuda.Event(), torch.cuda.Event()]
    main_stream = torch.cuda.current_stream()
    for e in ev_free:
        e.record(main_stream)

    def upload(k):
        """H2D of step k's features on the copy stream into buffer k % 2"""
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ev_free[k % 2])       # the step that last read this buffer is done
            dev_bufs[k % 2].copy_(host_feats, non_blocking=True)
            ev_ready[k % 2].record(copy_stream)

    def compute(k, resident):
        """one step = one costAndGrad over this rank's minibatch (+ the gradient all-reduce when
        data-parallel).  resident: features already in HBM (`feats`); else the copy-stream buffer"""
        if resident:
            src = feats
        else:
            main_stream.wait_event(ev_ready[k % 2])
            src = dev_bufs[k % 2]
        if dp is None:
            cost, grad, skip = net.costAndGradBatch(None, labels, feats_dev=src, T_b=Ts)
            if not resident:
                ev_free[k % 2].record(main_stream)
            return cost, skip
        # data-parallel: the step is queued without a host sync, the per-layer RCCL all-reduces
        # are queued behind the engine's gradient events (output layer first) and overlap the
        # rest of the backward pass; one sync at the end
        cost_dev, skip_dev = net.costAndGradBatchAsync(None, labels, feats_dev=src, T_b=Ts)
        if not resident:
            ev_free[k % 2].record(main_stream)
        dp.allreduce_gradients_overlapped(cost_dev, skip_dev)
        net.checkAsync()
        if dp.time_comm:
            cs = dp.comm_stats()
            if cs:
                comm_acc.append(cs)
        return cost_dev.cpu().numpy(), skip_dev.cpu().numpy().astype(bool)

    # roofline leg: asynchronous phase timers (sctc_brnn_set_profiling(h, 2)) -- one hipEvent per
    # kernel group on the compute stream, resolved after each step (every step ends in a host sync
    # anyway: the costs come back); no sync is added inside a step, so they run DURING the timed steps (--full only)
    Lp = _sctc.lib()
    if args.full:
        Lp.sctc_brnn_set_profiling(net._h, 2)
    phase_acc = np.zeros(len(PHASES))
    phase_arr = (ctypes.c_float * len(PHASES))()

    def run_steps(n, resident=True, collect=False):
        """n steps.  resident=False: the SURVEY 8(d) pipeline -- every step's features start in
        pinned host memory and are uploaded inside this call, overlapping the previous step"""
        step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        step_ev[0].record(main_stream)
        if not resident:
            upload(0)
        for k in range(n):
            if not resident and k + 1 < n:
                upload(k + 1)                               # overlaps compute(k)
            cost, skip = compute(k, resident)
            step_ev[k + 1].record(main_stream)
            if collect:
                Lp.sctc_brnn_phase_ms(net._h, phase_arr)
                phase_acc[:] += np.array(list(phase_arr))
        return cost, skip, step_ev

    def fence():
        torch.cuda.synchronize()
        if dp is not None:
            dist.barrier()
        torch.cuda.synchronize()

    comm_acc = []
    n1_ms = args.n1_ms
    if args.full and dp is not None and n1_ms is None:
        # what ONE GPU does alone with the same per-GPU minibatch (no exchange, HBM-resident features): every rank steps
        # on its own device at the same time, rank 0's figure is the N = 1 leg of scaling_efficiency_vs_n1
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        fence()
        t0 = time.perf_counter()
        for _ in range(max(3, args.steps // 2)):
            net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        torch.cuda.synchronize()
        n1_ms = (time.perf_counter() - t0) / max(3, args.steps // 2) * 1e3
        fence()
    if args.warmup:
        run_steps(args.warmup, resident=False)
    fence()
    if dp is not None and args.full:
        dp.time_comm = True
    t0 = time.perf_counter()
    cost, skip, step_ev = run_steps(args.steps, resident=False, collect=args.full)
    fence()
    elapsed = time.perf_counter() - t0
    if dp is not None:
        dp.time_comm = False
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, net, cost, skip)
    elapsed_res = 0.0
    if args.full:
        # side field: the same K steps with the features already resident in HBM
        run_steps(1, resident=True)
        fence()
        t0 = time.perf_counter()
        run_steps(args.steps, resident=True)
        fence()
        elapsed_res = time.perf_counter() - t0
    per_step_ms = sorted(step_ev[i].elapsed_time(step_ev[i + 1]) for i in range(args.steps))
    if dp is not None:
        t = torch.tensor([elapsed, elapsed_res], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, elapsed_res = float(t[0].item()), float(t[1].item())
    frames_total = world * B * T * args.steps
    ms_per_step = elapsed / args.steps * 1e3
    median_ms = per_step_ms[len(per_step_ms) // 2] if len(per_step_ms) % 2 else \
        0.5 * (per_step_ms[len(per_step_ms) // 2 - 1] + per_step_ms[len(per_step_ms) // 2])

    out = None
    if rank == 0:
        out = {
            "metric": "audio frames/sec (CTC fwd-bwd + BRNN grad) at T=1000, L=5, H=1824, |Sigma|=33",
            "value": frames_total / elapsed, "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "timing": {"value_is": "pinned_host_overlapped", "pinned_host_overlapped_ms": ms_per_step},
            "config": {"workload": "WSJ-shape cfg-3: T=1000 A=33 5x1824 BRNN (temporalLayer 3, "
                                   "inputDim 483) U=100, minibatch %d per GPU, one costAndGrad per "
                                   "step" % B,
                       "utterances_per_gpu": B, "frames_per_step": world * B * T,
                       "parallelism": ("dp%d (utterances sharded, per-layer RCCL all-reduce of the "
                                       "weight gradients overlapped with the backward pass)" % world)
                                      if dp is not None else "single-gpu",
                       "backend": backend if dp is not None else None,
                       "rccl_ranks": (["%d:%s:%s" % (r, i[0], i[1]) for r, i in enumerate(dp.device_ids)]
                                      if dp is not None else None),
                       "shared_device_mode": bool(dp.shared_device) if dp is not None else False},
            "ms_per_step_median": median_ms,
            "cost_mean": float(np.mean(cost[~skip])) if (~skip).any() else None,
        }
    if rank == 0 and args.full:
        # ---- roofline leg: the phase times of the K timed steps themselves
        L = _sctc.lib()
        ph = dict(zip(PHASES, [float(v) for v in phase_acc / max(1, args.steps)]))
        # cross-check: one extra step with the exact (synchronising) phase timers
        L.sctc_brnn_set_profiling(net._h, 1)
        arr = (ctypes.c_float * len(PHASES))()
        if dp is None:
            net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
            L.sctc_brnn_phase_ms(net._h, arr)
        ph_exact = dict(zip(PHASES, [float(v) for v in arr]))
        L.sctc_brnn_set_profiling(net._h, 0)
        tot, gm, rc = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        mb, keep = net._minibatch(feats, Ts, labels)
        L.sctc_brnn_flops(net._h, ctypes.byref(mb), ctypes.byref(tot), ctypes.byref(gm),
                          ctypes.byref(rc))
        gemm_ms = ph["fwd_gemm"] + ph["bwd_gemm"]
        rec_ms = ph["fwd_rec"] + ph["bwd_rec"]
        n_gemm_launches = (NL + 1) + (NL + 1) + NL + 2
        achieved = gm.value / (gemm_ms * 1e-3) / 1e12
        ctc_bytes = B * (2 * 4 * A * T + 4 * U + 8)
        out["timing"].update({"hbm_resident_ms": elapsed_res / args.steps * 1e3,
                              "hbm_resident_frames_per_s": frames_total / elapsed_res})
        out.update({
            "roofline": {"bound": "mfma", "kernel": "gemm_f32_kernel (all time-batched GEMMs)",
                         "achieved": achieved, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_F32_MFMA_TFLOPS, "traffic": None,
                         "measured": "live, inside the %d timed steps: one hipEvent per kernel group on the "
                                     "compute stream (sctc_brnn_set_profiling(h, 2): recorded asynchronously, "
                                     "resolved after each step, no sync added); phase_ms_exact_timers is one "
                                     "extra step with synchronising timers; profiles/r06_bench_kernel_stats.csv "
                                     "is rocprofv3's view of the same command" % args.steps,
                         "launches_per_step": n_gemm_launches,
                         "avg_launch_ms": gemm_ms / n_gemm_launches,
                         "algorithmic_tflop_per_step": gm.value / 1e12},
            "roofline_recurrent": {"bound": "latency (matrix pipes idle while the step hand-off crosses the fabric)", "kernel": "brnn_recurrent_q_kernel (two launches per step)",
                                   "achieved": rc.value / (rec_ms * 1e-3) / 1e12,
                                   "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                                   "frac": rc.value / (rec_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                                   "avg_launch_ms": rec_ms / 2, "us_per_time_step": rec_ms * 1e3 / (2 * (T - 1))},
            "roofline_ctc": {"bound": "hbm", "kernel": "softmax_rows + ctc_fused (alpha, beta and the gradient in one launch; "
                                                        "SCTC_CTC_FUSED=0: ctc_lattice + ctc_grad)",
                             "achieved": ctc_bytes / (ph["ctc"] * 1e-3) / 1e9, "peak": PEAK_HBM_GBPS,
                             "unit": "GB/s", "frac": ctc_bytes / (ph["ctc"] * 1e-3) / 1e9 / PEAK_HBM_GBPS,
                             "algorithmic_bytes": ctc_bytes, "ms": ph["ctc"]},
            "phase_ms": ph,
            "phase_ms_exact_timers": ph_exact,
            "timing_note": "SURVEY 8(d) pipeline: every step's features start in PINNED HOST memory, H2D "
                           "(%.1f MB per step) on a copy stream into one of two device buffers, "
                           "overlapping the previous step's compute, all K uploads inside the timed "
                           "region; value = frames / wall time of the K steps (barrier + synchronize on "
                           "both sides, max over ranks), median = hipEvent time between step ends; the "
                           "same K steps on HBM-resident features are the side field hbm_resident "
                           "(round 3 reported that one as value)" % (B * T * D * 4 / 1e6),
            "hbm_resident": {"value": frames_total / elapsed_res, "unit": "frames/s",
                             "ms_per_step": elapsed_res / args.steps * 1e3,
                             "note": "features resident in HBM when the timed region starts"},
        })
        out["cost_check"] = oracle_cost_check(cfg, net, host_feats[:T].numpy(), labels[0],
                                              float(cost[0]))
        # ---- side measurements (never `value`): SURVEY 8(d) defines the metric from pinned host
        # features, and asks for a second run with ragged lengths T_b ~ U[0.5T, T]
        # the 157.3 TFLOP/s figure assumes 2.4 GHz; register-only MFMA loops with fresh random
        # operands (no LDS / HBM traffic) show what the part sustains under realistic toggling
        probe = (ctypes.c_float * 8)()
        from tools.diag import sctc_diag       # hardware probes: not part of the product library
        if sctc_diag.lib().sctc_probe_mfma(probe, 8, None) == 0:
            out["roofline"]["sustained_peak"] = float(probe[4])
            out["roofline"]["frac_of_sustained"] = achieved / float(probe[4])
            out["roofline"]["sustained_note"] = ("v_mfma_f32_32x32x2_f32 loops on every SIMD: %.1f TFLOP/s "
                                                  "with constant operands, %.1f with random operands"
                                                  % (probe[0], probe[4]))
        # HBM-side traffic and MFMA-busy counters cannot be sampled from inside this process:
        # they come from the committed rocprofv3 --pmc passes of this same command
        # (tools/profile_bench.sh -> profiles/*_pmc_summary.json), labelled as such
        pmc = load_pmc_summary()
        if pmc and pmc.get("source_hash") != csrc_hash():
            out["roofline"]["traffic_note"] = (
                "%s was measured on other kernel sources (hash %s, running %s): not used; re-run "
                "tools/profile_bench.sh" % (pmc["_file"], pmc.get("source_hash"), csrc_hash()))
            pmc = None
        if pmc:
            g = pmc["kernels"].get("gemm_f32_kernel", {})
            if "fetch_bytes_x2" in g and "write_bytes" in g:
                out["roofline"]["traffic"] = g["fetch_bytes_x2"] + g["write_bytes"]
                out["roofline"]["traffic_note"] = (
                    "mean per gemm_f32_kernel launch, rocprofv3 FETCH_SIZE x2 (gfx950 wide-load "
                    "correction) + WRITE_SIZE from %s; algorithmic operand bytes per launch: %.3g"
                    % (pmc["_file"], gemm_operand_bytes(cfg) / n_gemm_launches))
            if "mfma_util" in g:
                out["roofline"]["mfma_util_pmc"] = g["mfma_util"]
            r = pmc["kernels"].get("brnn_recurrent", {})
            if "mfma_util" in r:
                out["roofline_recurrent"]["mfma_util_pmc"] = r["mfma_util"]
            c = pmc["kernels"]
            for trio in (("softmax_rows_kernel", "ctc_fused_kernel"),
                         ("softmax_rows_kernel", "ctc_lattice_kernel", "ctc_grad_kernel")):
                if all(k in c and "fetch_bytes" in c[k] and "write_bytes" in c[k] for k in trio):
                    raw = sum(c[k]["fetch_bytes"] + c[k]["write_bytes"] for k in trio)
                    out["roofline_ctc"]["traffic"] = raw
                    out["roofline_ctc"]["traffic_ratio"] = raw / ctc_bytes
                    out["roofline_ctc"]["traffic_kernels"] = list(trio)
                    out["roofline_ctc"]["traffic_note"] = (
                        "rocprofv3 FETCH_SIZE + WRITE_SIZE of %s, RAW: the guide's x2 correction of FETCH_SIZE is "
                        "calibrated for 16 B/lane reads only, these kernels read 4-16 B per lane (with x2 on the "
                        "fetches: %.3g bytes = %.1f x algorithmic); traffic_ratio = traffic / algorithmic_bytes"
                        % (" + ".join(trio), sum(c[k]["fetch_bytes_x2"] + c[k]["write_bytes"] for k in trio),
                           sum(c[k]["fetch_bytes_x2"] + c[k]["write_bytes"] for k in trio) / ctc_bytes))
                    break
            if out["roofline"].get("traffic"):
                out["roofline"]["traffic_ratio"] = out["roofline"]["traffic"] / (gemm_operand_bytes(cfg) / n_gemm_launches)
        if dp is not None:
            # where an N > 1 step's time goes besides compute: the overlapped exchange of the weight gradients
            # (dist_sgd.comm_stats; rank 0's view, mean over the timed steps) and the same per-GPU work on one GPU alone
            if comm_acc:
                out["comm"] = {k: (comm_acc[0][k] if k in ("bytes", "buckets") else float(np.mean([c[k] for c in comm_acc])))
                               for k in comm_acc[0]}
                out["comm"]["note"] = ("per step, rank 0, mean of %d timed steps: allreduce_ms = first layer's gradient final -> "
                                       "last collective finished (side stream; includes waiting for later layers), exposed_ms = "
                                       "how far that lies behind the end of the backward pass (not hidden), busbw = bytes / "
                                       "allreduce_ms x 2 (N - 1) / N" % len(comm_acc))
            res_ms = elapsed_res / args.steps * 1e3
            out["scaling_efficiency_vs_n1"] = {"value": n1_ms / res_ms if res_ms > 0 else None, "n1_ms": n1_ms,
                                               "n_ms": res_ms,
                                               "n1_source": "--n1-ms" if args.n1_ms is not None else "measured in this run (rank 0 alone on its GPU, no exchange)",
                                               "note": "weak scaling, HBM-resident features on both sides: per-GPU work is fixed, so the efficiency "
                                                       "is the single-GPU step time over the N-GPU step time"}
        if dp is None and not args.no_side:
            side_measurements(out, net, feats, labels, Ts, rs, torch, B, T, D)
            recurrent_by_minibatch(out, torch, cfg)
            gemm_frac_with_separate_sums(out, torch, cfg, labels, feats)
            f32_split_bf16x3(out, torch, cfg, labels, feats, net)
            ctc_saturation(out, torch, A, T, U)
            ctc_long_rows(out, torch)
            del net, feats, dev_bufs
            torch.cuda.empty_cache()
            small_configs(out, torch)
            cfg4_share(out, torch)
            cfg5_fp16(out, torch)
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
    if dp is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


def load_pmc_summary():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            d = json.load(f)
        d["_file"] = os.path.relpath(files[-1], ROOT)
        return d
    except Exception:
        return None


def gemm_operand_bytes(cfg):
    """algorithmic bytes the time-batched GEMMs of one step must move once: every operand and
    result matrix read/written one time (fwd, dgrad, wgrad, recurrent wgrad), fp32"""
    D, A, H, NL, T, B = (cfg[k] for k in ("D", "A", "H", "NL", "T", "B"))
    rows = B * T
    dims = [D] + [H] * NL + [A]
    total = 0
    for i in range(NL + 1):
        m, n = dims[i + 1], dims[i]
        total += (rows * n + m * n + rows * m)            # fwd: X, W -> Z
        total += (rows * m + rows * n + m * n)            # wgrad: delta, X -> dW
        if i > 0:
            total += (rows * m + m * n + rows * n)        # dgrad: delta, W -> dX
    total += 2 * (2 * rows * H + H * H)                   # recurrent wgrads
    return 4 * total


def side_measurements(out, net, feats, labels, Ts, rs, torch, B, T, D):
    """never `value`: the NON-overlapped PCIe rate (what the double buffering buys) and the
    ragged-minibatch rate SURVEY 8(d) asks for beside the headline"""
    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    host_feats = torch.empty(B * T, D, dtype=torch.float32).pin_memory()
    host_feats.copy_(feats)
    dt = timed(lambda: net.costAndGradBatch(None, labels, feats_dev=host_feats.cuda(non_blocking=True), T_b=Ts), 3)
    out["pcie_serial"] = {"value": B * T / dt, "unit": "frames/s", "ms_per_step": dt * 1e3,
                          "h2d_bytes_per_step": B * T * D * 4,
                          "note": "H2D on the compute stream, not overlapped"}
    Tr = sorted((int(t) for t in rs.randint(T // 2, T + 1, size=B)), reverse=True)
    lab_r = [l[:max(1, t // 10)] for l, t in zip(labels, Tr)]
    feats_r = feats[:sum(Tr)]
    dt = timed(lambda: net.costAndGradBatch(None, lab_r, feats_dev=feats_r, T_b=Tr), 3)
    out["ragged"] = {"value": sum(Tr) / dt, "unit": "frames/s", "ms_per_step": dt * 1e3,
                     "frames_per_step": sum(Tr),
                     "note": "T_b ~ U[T/2, T] sorted descending, U_b = T_b/10, same net, HBM-resident"}
    # the reference's mode: minibatch 1, one call per utterance
    n1 = 4
    dt = timed(lambda: [net.costAndGradBatch(None, [labels[i]], feats_dev=feats[i * T:(i + 1) * T], T_b=[T])
                        for i in range(n1)], 2)
    out["one_utterance_per_call"] = {
        "value": n1 * T / dt, "unit": "frames/s", "ms_per_utterance": dt * 1e3 / n1,
        "note": "the reference's mode (minibatch 1), one synchronous call per utterance"}
    # north_star "a minibatch of utterances shards one-utterance-per-stream on one GPU": minibatch-1
    # steps on n HIP streams, their kernels overlapping on the device (NNet.costAndGradStreams; two
    # 228-workgroup grids of the small-batch persistent recurrence fit the part side by side)
    n8 = min(8, B)
    per = {}
    for ns in (1, 2, 3, 4):
        dt = timed(lambda: net.costAndGradStreams(None, labels[:n8], n_streams=ns, feats_dev=feats[:n8 * T],
                                                  T_b=[T] * n8), 2)
        per[ns] = n8 * T / dt
    best_ns = max(per, key=per.get)
    out["one_utterance_per_stream"] = {
        "value": per[best_ns], "unit": "frames/s", "streams": best_ns, "utterances": n8,
        "by_streams": {str(k): v for k, v in per.items()},
        "note": "every utterance its own minibatch-1 costAndGrad on one of n HIP streams, gradients "
                "summed; the packed time-major minibatch (`value`) is the faster way to use the part"}


def recurrent_by_minibatch(out, torch, cfg):
    """MFMA utilisation of the recurrent TIME-STEP contraction as a function of the
    minibatch (the time-batched GEMMs are `roofline`).  cfg-3 layer sizes, utterances of T/4 frames (a
    time step costs the same at any T), one profiled step per size; FLOPs = 2 directions x (2 H^2 B
    forward + 2 H^2 B BPTT) per time step, against the dense fp32 MFMA peak."""
    from nnets import brnnet
    import _sctc
    D, A, H, NL, TL = (cfg[k] for k in ("D", "A", "H", "NL", "TL"))
    T = max(64, cfg["T"] // 4)
    L = _sctc.lib()
    res = {}
    for B in (16, 32, 64, 128):
        np.random.seed(0)
        net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B)
        net.initParams()
        g = torch.Generator(device="cuda")
        g.manual_seed(9)
        feats = torch.randn(B * T, D, device="cuda", generator=g)
        rs = np.random.RandomState(9)
        labels = [rs.randint(1, A, size=max(1, T // 10)).astype(np.int32) for _ in range(B)]
        Ts = [T] * B
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        L.sctc_brnn_set_profiling(net._h, 1)
        acc = np.zeros(len(PHASES))
        arr = (ctypes.c_float * len(PHASES))()
        n = 3
        for _ in range(n):
            net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
            L.sctc_brnn_phase_ms(net._h, arr)
            acc += np.array(list(arr))
        L.sctc_brnn_set_profiling(net._h, 0)
        ph = dict(zip(PHASES, acc / n))
        us = (ph["fwd_rec"] + ph["bwd_rec"]) * 1e3 / (2 * (T - 1))
        flops_per_time_step = 2 * 2.0 * H * H * B          # both directions, one pass
        res[str(B)] = {"us_per_time_step": us, "tflops": flops_per_time_step / (us * 1e-6) / 1e12,
                       "frac_of_f32_mfma_peak": flops_per_time_step / (us * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                       "path": list(net.recurrentPath())}
        del net, feats
        torch.cuda.empty_cache()
    out["roofline_recurrent"]["by_minibatch"] = res
    # the whole cfg-3 step at 128 utterances of the full length (HBM-resident features): what the larger minibatch buys
    # once the recurrence runs the units x utterances kernel (round 6) -- a side field, never `value`
    B, T = 128, cfg["T"]
    np.random.seed(0)
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B)
    net.initParams()
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    feats = torch.randn(B * T, D, device="cuda", generator=g)
    rs = np.random.RandomState(9)
    labels = [rs.randint(1, A, size=max(1, T // 10)).astype(np.int32) for _ in range(B)]
    Ts = [T] * B
    net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 3
    for _ in range(n):
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    out["minibatch_128"] = {"value": B * T / dt, "unit": "frames/s", "ms_per_step": dt * 1e3, "utterances": B, "T": T,
                            "features": "HBM-resident", "recurrent_path": list(net.recurrentPath())}
    del net, feats
    torch.cuda.empty_cache()


def ctc_saturation(out, torch, A, T, U):
    """roofline_ctc beside the headline minibatch: the CTC kernels alone at the batch that
    saturates them (4096 utterances of the cfg-3 shape), float32 probabilities on the device"""
    import ctc_fast
    import _sctc
    B = 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    probs = torch.softmax(torch.randn(B * T, A, device="cuda", generator=g), dim=1)
    rs = np.random.RandomState(7)
    seqs = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
    ctc_fast.ctc_loss_batch(probs, seqs, lengths=[T] * B)
    torch.cuda.synchronize()
    # (a) the Python entry as a caller uses it; (b) the C entry alone on prepared host arrays, between two events:
    # descriptor build + pinned upload + kernel
    best_wall, best_gpu = 1e9, 1e9
    labels = np.concatenate(seqs)
    U_b = np.full(B, U, dtype=np.int32)
    T_b = np.full(B, T, dtype=np.int32)
    label_off = (np.arange(B, dtype=np.int64) * U)
    frame_off = (np.arange(B, dtype=np.int64) * T)
    grad = torch.empty_like(probs)
    for _ in range(3):
        t0 = time.perf_counter()
        ctc_fast.ctc_loss_batch(probs, seqs, lengths=[T] * B)
        torch.cuda.synchronize()
        best_wall = min(best_wall, time.perf_counter() - t0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctc_fast._run_batch(probs, grad, A, probs.shape[1], 0, T_b, U_b, frame_off, labels, label_off, _sctc.F32)
        e1.record()
        torch.cuda.synchronize()
        best_gpu = min(best_gpu, e0.elapsed_time(e1) * 1e-3)
    byts = B * (2 * 4 * A * T + 4 * U + 8)
    out["roofline_ctc"]["saturating_batch"] = {
        "utterances": B, "ms": best_gpu * 1e3, "achieved": byts / best_gpu / 1e9, "unit": "GB/s",
        "frac": byts / best_gpu / 1e9 / PEAK_HBM_GBPS,
        "ms_wall": best_wall * 1e3, "achieved_wall": byts / best_wall / 1e9,
        "note": "ctc_fused_kernel (two waves per utterance at this batch) on 4096 utterances of T=%d U=%d, float32 "
                "probabilities resident on the device: `ms` between two events around the C entry sctc_ctc_loss_batch "
                "(workspace allocation, descriptor build and pinned upload, kernel; the kernel alone: profiles/"
                "r06_ctc_paths_kernel_stats.csv), `ms_wall` the Python entry ctc_loss_batch with its 4096 label arrays "
                "(rounds 1-4 reported that one: 11.4 ms with the three-kernel path).  The float64 recursion is "
                "latency/issue-bound, not HBM-bound (DESIGN.md 4.3)" % (T, U)}
    # Which bound it IS on cannot be sampled from inside this process: the SQ counters of the same kernel at the same batch
    # come from the committed rocprofv3 --pmc passes (tools/profile_ctc_bound.sh -> profiles/r*_ctc_bound_sat.json),
    # read back only if they were measured on these CTC sources
    import glob
    import hashlib
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_ctc_bound_sat.json")))
    if files:
        pm = json.load(open(files[-1]))
        h = hashlib.sha256()
        for f in ("ctc_fused.hip", "ctc_store.h", "ctc_kernels.h", "xlane.h", "common.h"):
            h.update(open(os.path.join(ROOT, "stanford-ctc_amd", "csrc", f), "rb").read())
        sat = out["roofline_ctc"]["saturating_batch"]
        if pm.get("source_hash_ctc") != h.hexdigest()[:16]:
            sat["bound_note"] = "%s was measured on other CTC sources: not used; re-run tools/profile_ctc_bound.sh" % os.path.basename(files[-1])
        else:
            k = [v for n, v in pm["kernels"].items() if "ctc_fused_kernel" in n]
            if k:
                k = k[0]
                util = k.get("simd_valu_util")
                sat["valu_busy"] = util
                sat["bound"] = ("fp64-issue" if util is not None and util >= 0.8 else
                                "latency" if util is not None and util < 0.6 else "issue + latency")
                sat["counters"] = {"simd_valu_util": util, "wave_valu_busy": k.get("valu_busy"), "wave_issue_busy": k.get("issue_busy"),
                                   "wave_parked": k.get("parked"), "wave_issue_stalled": k.get("issue_stalled"),
                                   "float64_share_of_valu_instructions": k.get("float64_share_of_valu_instructions"),
                                   "valu_instructions_per_wave_and_frame": k["per_wave"]["valu"] / T if "per_wave" in k else None,
                                   "shader_clock_GHz_while_profiled": k.get("shader_clock_GHz_while_profiled"),
                                   "source": os.path.basename(files[-1])}
                sat["bound_note"] = ("SQ counters of ctc_fused_kernel at this batch (rocprofv3 --pmc, %s): the device's SIMDs execute a VALU "
                                     "instruction in valu_busy of their cycles with three recursion waves per SIMD (168 registers; round 5: two, 194, "
                                     "0.64); a wave has one "
                                     "executing in wave_valu_busy of its resident time, waits at s_waitcnt / barriers in wave_parked and on "
                                     "dependencies in wave_issue_stalled: neither the float64 pipe's issue slots (>= 0.8) nor latency alone (< 0.6) -- "
                                     "HBM is not the bound at any batch" % os.path.basename(files[-1]))
                out["roofline_ctc"]["bound"] = "issue + latency (float64 recursion; see saturating_batch.bound / valu_busy); HBM fraction reported for the record"


def ctc_long_rows(out, torch):
    """roofline_ctc.long_rows: label rows of 1601 lattice states (the cfg-5 shape, T = 8000 / U = 800) at 32 utterances --
    the wide fused kernel (ctc_fusedw.hip, the default from 18 utterances on) beside the lattice + grad kernels it
    replaces there (SCTC_CTC_WIDE=0), events around the Python entry on device-resident float32 probabilities"""
    import ctc_fast
    A, T, U, B = 33, 8000, 800, 32
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    probs = torch.softmax(torch.randn(B * T, A, device="cuda", generator=g), dim=1)
    rs = np.random.RandomState(7)
    seqs = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
    ms, cost = {}, {}
    old = os.environ.get("SCTC_CTC_WIDE")
    try:
        for name, env in (("wide", None), ("lattice_grad", "0")):
            os.environ.pop("SCTC_CTC_WIDE", None)
            if env is not None:
                os.environ["SCTC_CTC_WIDE"] = env
            c, _, _ = ctc_fast.ctc_loss_batch(probs, seqs, lengths=[T] * B)
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c, _, _ = ctc_fast.ctc_loss_batch(probs, seqs, lengths=[T] * B)
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1))
            ms[name] = best
            cost[name] = np.asarray(c.cpu() if hasattr(c, "cpu") else c, dtype=np.float64)
            torch.cuda.empty_cache()
    finally:
        os.environ.pop("SCTC_CTC_WIDE", None)
        if old is not None:
            os.environ["SCTC_CTC_WIDE"] = old
    byts = B * (2 * 4 * A * T + 4 * U + 8)
    out["roofline_ctc"]["long_rows"] = {
        "shape": "T=8000 U=800 (1601 lattice states), %d symbols" % A, "utterances": B,
        "ms": ms["wide"], "achieved": byts / (ms["wide"] * 1e-3) / 1e9, "unit": "GB/s",
        "ms_lattice_grad": ms["lattice_grad"], "achieved_lattice_grad": byts / (ms["lattice_grad"] * 1e-3) / 1e9,
        "max_cost_rel_distance": float(np.max(np.abs(cost["wide"] - cost["lattice_grad"]) / np.abs(cost["lattice_grad"]))),
        "note": "ctc_fusedw_kernel (meet in the middle on 8 waves per direction, one packed 32-bit row store; default from 18 "
                "utterances on) against ctc_lattice_kernel + ctc_grad_kernel (two float64 lattices; SCTC_CTC_WIDE=0) on the same "
                "batch; HBM traffic of the two: profiles/r06_ctc_traffic_cfg5.txt (37x against 175x algorithmic at 8 utterances)"}
    del probs
    torch.cuda.empty_cache()


def f32_split_bf16x3(out, torch, cfg, labels, feats, net32):
    """The headline workload with the time-batched contractions on the bfloat16 matrix cores: every
    fp32 operand split exactly into three bfloat16 terms, six cross products, fp32 accumulation
    (NNet(..., gemm="bf16x3"), gemm_s3.hip).  fp32-accurate -- the error against a float64 product
    equals the fp32 fma chain's (tests/test_gpu_bf16x3.py) -- but NOT the reference's instruction, so
    it is opt-in and a side field, never `value`."""
    from nnets import brnnet
    import _sctc
    D, A, H, NL, TL, T, U, B = (cfg[k] for k in ("D", "A", "H", "NL", "TL", "T", "U", "B"))
    np.random.seed(0)
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B, gemm="bf16x3")
    net.initParams()                        # same seed -> the same weights as the fp32 net
    Ts = [T] * B
    c32, _, _ = net32.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    g32 = net32.grad.flat.clone()
    c3, _, _ = net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    g3 = net.grad.flat
    gdiff = float((g3 - g32).double().norm() / g32.double().norm())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 5
    for _ in range(n):
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    L = _sctc.lib()
    L.sctc_brnn_set_profiling(net._h, 1)
    net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    arr = (ctypes.c_float * len(PHASES))()
    L.sctc_brnn_phase_ms(net._h, arr)
    L.sctc_brnn_set_profiling(net._h, 0)
    ph = dict(zip(PHASES, [float(v) for v in arr]))
    tot, gm, rc = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    mb, keep = net._minibatch(feats, Ts, labels)
    L.sctc_brnn_flops(net._h, ctypes.byref(mb), ctypes.byref(tot), ctypes.byref(gm), ctypes.byref(rc))
    gemm_ms = ph["fwd_gemm"] + ph["bwd_gemm"]
    ach = gm.value / (gemm_ms * 1e-3) / 1e12
    out["f32_split_bf16x3"] = {
        "workload": "the headline workload (cfg-3, minibatch %d, HBM-resident features), gemm='bf16x3'" % B,
        "dtype": "f32 operands and results; products as 6 bf16 x bf16 terms of an exact 3-term split, f32 accumulate",
        "value": B * T / dt, "unit": "frames/s", "ms_per_step": dt * 1e3, "phase_ms": ph,
        "cost_rel_err_vs_float64_oracle": abs(float(c3[0]) - out["cost_check"]["oracle"]) / abs(out["cost_check"]["oracle"]),
        "max_cost_rel_diff_vs_f32_path": float(np.max(np.abs(c3 - c32) / np.abs(c32))),
        "grad_rel_norm_diff_vs_f32_path": gdiff,
        "roofline_gemm": {"bound": "mfma + lds", "kernel": "gemm_s3_kernel",
                          "achieved": ach, "unit": "TFLOP/s (algorithmic fp32 flops)",
                          "peak": PEAK_F16_MFMA_TFLOPS / 6.0, "frac": ach / (PEAK_F16_MFMA_TFLOPS / 6.0),
                          "note": "peak = dense bf16 MFMA peak / 6 executed products per algorithmic product; "
                                  "a register-only loop of v_mfma_f32_32x32x16_bf16 on random operands sustains "
                                  "1775 TFLOP/s (tools/valu_rate.hip), i.e. 296 fp32-equivalent; the forward kernel keeps "
                                  "the matrix cores 76 % busy at a shader clock of 1.44 GHz (power-bound), DESIGN.md 4.1c"}}
    del net


def gemm_frac_with_separate_sums(out, torch, cfg, labels, feats):
    """roofline.frac once more with the two sums around the temporal layer (hActsFor + hActsBack, deltasFor +
    deltasBack) in their own add_kernel launches (SCTC_FUSE_ADD=0) instead of inside two of the GEMM launches: the
    GEMM group then carries 0.22 ms less work per step and add_kernel shows up under `other` -- same step time
    (0.695 fused vs 0.71 unfused is bookkeeping, this puts both in the line)."""
    from nnets import brnnet
    import _sctc
    D, A, H, NL, TL, T, U, B = (cfg[k] for k in ("D", "A", "H", "NL", "TL", "T", "U", "B"))
    old = os.environ.get("SCTC_FUSE_ADD")
    os.environ["SCTC_FUSE_ADD"] = "0"
    try:
        np.random.seed(0)
        net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B, gemm="f32")
        net.initParams()
    finally:
        if old is None:
            del os.environ["SCTC_FUSE_ADD"]
        else:
            os.environ["SCTC_FUSE_ADD"] = old
    Ts = [T] * B
    L = _sctc.lib()
    L.sctc_brnn_set_profiling(net._h, 2)
    arr = (ctypes.c_float * len(PHASES))()
    acc = np.zeros(len(PHASES))
    net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 5
    for _ in range(n):
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        L.sctc_brnn_phase_ms(net._h, arr)
        acc += np.array([float(v) for v in arr])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    L.sctc_brnn_set_profiling(net._h, 0)
    ph = dict(zip(PHASES, (acc / n).tolist()))
    tot, gm, rc = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    mb, keep = net._minibatch(feats, Ts, labels)
    L.sctc_brnn_flops(net._h, ctypes.byref(mb), ctypes.byref(tot), ctypes.byref(gm), ctypes.byref(rc))
    gemm_ms = ph["fwd_gemm"] + ph["bwd_gemm"]
    ach = gm.value / (gemm_ms * 1e-3) / 1e12
    out["roofline"]["sums_in_add_kernel"] = {
        "frac": ach / PEAK_F32_MFMA_TFLOPS, "achieved": ach, "gemm_ms": gemm_ms, "other_ms": ph["other"],
        "ms_per_step": dt * 1e3,
        "note": "SCTC_FUSE_ADD=0, HBM-resident features: the same GEMM flops with the two sums around the temporal "
                "layer in add_kernel (2 launches, counted under `other`) instead of inside 2 of the %d GEMM launches"
                % ((NL + 1) + (NL + 1) + NL + 2)}
    del net


def cfg5_fp16(out, torch):
    """BASELINE configs[4] as specified: T=8000 A=33 7x2048 (temporalLayer 4, inputDim 615) U=800,
    fp16 operands / fp32 accumulate / float64 CTC, minibatch 8 and 1 -- a side field, never `value`"""
    from nnets import brnnet
    import _sctc
    D, A, H, NL, TL, T, U = 615, 33, 2048, 7, 4, 8000, 800
    res = {}
    for B in (8, 1):
        np.random.seed(0)
        net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B, fp16=True)
        net.initParams()
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        feats = torch.randn(B * T, D, device="cuda", generator=g)
        rs = np.random.RandomState(5)
        labels = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
        Ts = [T] * B
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 3
        L = _sctc.lib()
        L.sctc_brnn_set_profiling(net._h, 1)
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
        arr = (ctypes.c_float * len(PHASES))()
        L.sctc_brnn_phase_ms(net._h, arr)
        L.sctc_brnn_set_profiling(net._h, 0)
        ph = dict(zip(PHASES, [float(v) for v in arr]))
        tot, gm, rc = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        mb, keep = net._minibatch(feats, Ts, labels)
        L.sctc_brnn_flops(net._h, ctypes.byref(mb), ctypes.byref(tot), ctypes.byref(gm), ctypes.byref(rc))
        gemm_ms = ph["fwd_gemm"] + ph["bwd_gemm"]
        res["minibatch_%d" % B] = {
            "value": B * T / dt, "unit": "frames/s", "ms_per_step": dt * 1e3, "phase_ms": ph,
            "roofline_gemm": {"bound": "mfma", "kernel": "gemm_g16_kernel (LDS-DMA; gemm_x16_kernel for the gathered / small shapes): f16 fwd / bf16 bwd shadow operands, f32 accumulate",
                              "achieved": gm.value / (gemm_ms * 1e-3) / 1e12, "peak": PEAK_F16_MFMA_TFLOPS,
                              "unit": "TFLOP/s", "frac": gm.value / (gemm_ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS,
                              "note": "16-bit shadow copies of activations / deltas / weights are written by "
                                      "their producers; the kernel is bound by the CU's operand-load path "
                                      "(DESIGN.md 4.1b), not by the matrix pipes"},
            "us_per_recurrent_step": (ph["fwd_rec"] + ph["bwd_rec"]) * 1e3 / (2 * (T - 1)),
            "ctc_ms": ph["ctc"]}
        del net
        torch.cuda.empty_cache()
    out["cfg5_fp16"] = {"workload": "cfg-5: T=8000 A=33 7x2048 BRNN (temporalLayer 4, inputDim 615) U=800, "
                                    "operand_dtype fp16 (float16 forward / bfloat16 backward operands, fp32 "
                                    "accumulate, float64 CTC lattices), HBM-resident features",
                        "dtype": "f16 operands / f32 accumulate", **res}


def small_configs(out, torch):
    """BASELINE configs[0] and [1] at their real sizes, minibatch 1 (the reference's own mode: one utterance per
    costAndGrad call): T=200 A=28 2x512 (temporalLayer 1, inputDim 615) U=20 and the TIMIT shape T=300 A=62 3x1024
    (temporalLayer 2, inputDim 943) U=30, fp32, HBM-resident features -- side fields, never `value`.  They are
    launch- and latency-bound (a step is 0.5-1 ms of 40-odd launches and 2 x (T - 1) dependent recurrent steps)."""
    from nnets import brnnet
    import _sctc
    L = _sctc.lib()
    for name, (D, A, H, NL, TL, T, U) in (("cfg1_minibatch1", (615, 28, 512, 2, 1, 200, 20)),
                                           ("cfg2_minibatch1", (943, 62, 1024, 3, 2, 300, 30))):
        np.random.seed(0)
        net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=1, gemm="f32")
        net.initParams()
        g = torch.Generator(device="cuda")
        g.manual_seed(2)
        feats = torch.randn(T, D, device="cuda", generator=g)
        rs = np.random.RandomState(2)
        labels = [rs.randint(1, A, size=U).astype(np.int32)]
        for _ in range(3):
            net.costAndGradBatch(None, labels, feats_dev=feats, T_b=[T])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 20
        for _ in range(n):
            net.costAndGradBatch(None, labels, feats_dev=feats, T_b=[T])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        L.sctc_brnn_set_profiling(net._h, 1)
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=[T])
        arr = (ctypes.c_float * len(PHASES))()
        L.sctc_brnn_phase_ms(net._h, arr)
        L.sctc_brnn_set_profiling(net._h, 0)
        ph = dict(zip(PHASES, [float(v) for v in arr]))
        out[name] = {"workload": "T=%d A=%d %dx%d BRNN (temporalLayer %d, inputDim %d) U=%d, minibatch 1, fp32" % (T, A, NL, H, TL, D, U),
                     "value": T / dt, "unit": "frames/s", "ms_per_utterance": dt * 1e3, "phase_ms": ph,
                     "us_per_recurrent_step": (ph["fwd_rec"] + ph["bwd_rec"]) * 1e3 / (2 * (T - 1))}
        del net, feats
    torch.cuda.empty_cache()


def cfg4_share(out, torch):
    """BASELINE configs[3] (SWBD shape, minibatch 256 over 8 GPUs): ONE GPU's share -- 32 utterances of T=2000, A=33,
    5x1824 (temporalLayer 3, inputDim 615), U=200, fp32 -- as a side field, never `value`.  It is the N = 1 leg of the
    weak-scaling run `bench.py --gpus 8` would do on that configuration; its 401-state label rows take the fused CTC
    kernel with 8 states per lane."""
    from nnets import brnnet
    import _sctc
    D, A, H, NL, TL, T, U, B = 615, 33, 1824, 5, 3, 2000, 200, 32
    np.random.seed(0)
    net = brnnet.NNet(D, A, H, NL, T, temporalLayer=TL, maxUtts=B, gemm="f32")
    net.initParams()
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    feats = torch.randn(B * T, D, device="cuda", generator=g)
    rs = np.random.RandomState(4)
    labels = [rs.randint(1, A, size=U).astype(np.int32) for _ in range(B)]
    Ts = [T] * B
    net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 3
    for _ in range(n):
        net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    L = _sctc.lib()
    L.sctc_brnn_set_profiling(net._h, 1)
    net.costAndGradBatch(None, labels, feats_dev=feats, T_b=Ts)
    arr = (ctypes.c_float * len(PHASES))()
    L.sctc_brnn_phase_ms(net._h, arr)
    L.sctc_brnn_set_profiling(net._h, 0)
    ph = dict(zip(PHASES, [float(v) for v in arr]))
    out["cfg4_share"] = {"workload": "cfg-4, one GPU's share of the 8-GPU minibatch 256: 32 utterances of T=2000 A=33 5x1824 BRNN "
                                     "(temporalLayer 3, inputDim 615) U=200, fp32, HBM-resident features",
                         "value": B * T / dt, "unit": "frames/s", "ms_per_step": dt * 1e3, "phase_ms": ph,
                         "ctc_ms": ph["ctc"], "us_per_recurrent_step": (ph["fwd_rec"] + ph["bwd_rec"]) * 1e3 / (2 * (T - 1)),
                         "note": "what each of 8 ranks would do per step before the RCCL all-reduce of the 20.9 M-parameter gradient; "
                                 "no 8-GPU node was available to any round (DESIGN.md 7)"}
    del net, feats
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
