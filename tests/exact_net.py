"""Integer-grid BRNN cases whose arithmetic is exact, and a batched float64 reference (TEST HELPER, no tests).

Every feature, weight, bias and the activation ceiling of a case is a small integer (the output layer: an integer
times one power of two), so every product and every partial sum of every hidden layer is an integer far below 2^24:
fp32 accumulation gives the mathematically exact value in ANY summation order, for any K split, on any MFMA shape, and
the 16-bit operand paths are exact too (integers <= 2048 are float16 values).  hActsFor / hActsBack of every kernel
and operand mode must therefore be BIT-equal to the float64 oracle, every (0, maxAct) mask is the same in all
implementations, and the backward pass is a fixed linear map of the CTC delta.

make_case()   one case, with the conditions that keep it from being vacuous asserted on the float64 reference alone
reference()   forward and (given oracle.ctc's per-utterance deltas) backward pass, one (H x H) @ (H x B_active)
              product per time step and direction instead of a loop over utterances
Rounding      where the fp16-operand configuration rounds in its backward pass; reference(mixed=Rounding(..)) restates it:
              with float64 accumulation it is the model the device is compared with, with float32 its noise estimate
GPU_CASES     the matrix of tests/test_gpu_recurrence_exact.py (the CPU suite checks make_case's conditions on it)
and the comparisons both suites use: forward_rows_differing() (bit equality after the cast to float32, counted per
(utterance, frame) row), row_errors() (per-frame relative error of a delta matrix) and, for the fp16-operand backward
pass, mixed_stats() / mixed_e_ref() / mixed_violations().

Columns of every internal matrix are PACKED time-major like the engine's rows: frame t of the utterance with length
rank r (stable sort by length, longest first) is column rowbase[t] + r, so the utterances alive at a step are one
contiguous slice.  What reference() returns is per utterance, in the caller's order, in the oracle's (features, T)
layout.
"""
import collections
import functools
from types import SimpleNamespace

import numpy as np

from oracle import brnn as obrnn
from oracle import ctc as octc

MAX_ACT = 20.0
REC_NNZ = 32          # non-zeros (+-1) per row of Wf / Wb
FF_NNZ = 16           # non-zeros (+-1) per row of a hidden (H x H) feed-forward layer: |z| <= 16 * 40 + |b| < 2048


# ------------------------------------------------------------------ generator

def _sparse_sign(rs, rows, cols, nnz):
    """(rows, cols) float64 matrix, `nnz` entries per row at random columns, half of them +1 and half -1: with
    balanced rows no unit's recurrent input has a mean that pins it to one side of the clip for a whole case"""
    k = min(nnz, cols)
    idx = np.argpartition(rs.rand(rows, cols), k - 1, axis=1)[:, :k]
    sign = np.where(np.argsort(rs.rand(rows, k), axis=1) % 2 == 0, 1.0, -1.0)
    W = np.zeros((rows, cols))
    np.put_along_axis(W, idx, sign, axis=1)
    return W


def empty_blocks(W, blk=16):
    """(row block, column block) indices of the blk x blk blocks of W (edge blocks partial) without a non-zero"""
    R, C = W.shape
    Rp, Cp = -(-R // blk) * blk, -(-C // blk) * blk
    P = np.zeros((Rp, Cp), dtype=bool)
    P[:R, :C] = W != 0
    any_nz = P.reshape(Rp // blk, blk, Cp // blk, blk).any(axis=(1, 3))
    return np.argwhere(~any_nz)


def _plant_blocks(rs, W, blk=16):
    """a +-1 where chance left a 16 x 16 block empty: no K chunk of any row block of any kernel is multiplied by zeros only"""
    R, C = W.shape
    for i, j in empty_blocks(W, blk):
        r = i * blk + rs.randint(0, min(blk, R - i * blk))
        c = j * blk + rs.randint(0, min(blk, C - j * blk))
        W[r, c] = rs.choice([-1.0, 1.0])
    return W


def _ragged_lengths(rs, B, Tmax):
    """1..Tmax, at least one utterance of one frame and two of Tmax frames (B >= 3; B = 2: one of each; B = 1: Tmax),
    in an order that is not sorted"""
    if B == 1:
        return [Tmax]
    if B == 2:
        return [1, Tmax]
    # few utterances: the free lengths from the upper half, so that the case has frames enough for every unit to open once
    Ts = [1, Tmax, Tmax] + [int(t) for t in rs.randint(Tmax // 2 if B <= 8 else 1, Tmax + 1, size=B - 3)]
    while True:
        rs.shuffle(Ts)
        if Ts != sorted(Ts) and Ts != sorted(Ts, reverse=True):
            return Ts


def _labels(rs, T, A):
    """max(1, T // 3) labels in 1..A-1, no immediate repeat (always feasible in T frames)"""
    U = max(1, T // 3)
    lab = [int(rs.randint(1, A))]
    for _ in range(U - 1):
        lab.append(1 + (lab[-1] - 1 + int(rs.randint(1, A - 1))) % (A - 1))
    return np.array(lab, dtype=np.int32)


def plan(Ts):
    """the engine's packing: order (rank -> caller index, stable by length, longest first), rank (its inverse),
    rowbase[t], nact[t] and cols[b] = the packed columns of caller utterance b's frames"""
    Ts = [int(t) for t in Ts]
    B = len(Ts)
    order = sorted(range(B), key=lambda b: -Ts[b])
    rank = np.empty(B, dtype=np.int64)
    rank[order] = np.arange(B)
    Tmax = Ts[order[0]]
    Tsorted = np.array([Ts[b] for b in order])
    nact = np.array([(Tsorted > t).sum() for t in range(Tmax)], dtype=np.int64)
    rowbase = np.concatenate([[0], np.cumsum(nact)[:-1]]).astype(np.int64)
    cols = [rowbase[:Ts[b]] + rank[b] for b in range(B)]
    return SimpleNamespace(B=B, Ts=Ts, Tmax=Tmax, order=order, rank=rank, nact=nact, rowbase=rowbase, cols=cols,
                           N=int(nact.sum()))


def _pack(mats, pl, rows):
    out = np.zeros((rows, pl.N))
    for b, m in enumerate(mats):
        out[:, pl.cols[b]] = m
    return out


def _unpack(M, pl):
    return [np.array(M[:, pl.cols[b]]) for b in range(pl.B)]


@functools.lru_cache(maxsize=4)          # (a large case holds a few hundred MB)
def make_case(H, B, NL=2, TL=1, Tmax=14, seed=0, D=16, A=9):
    """-> case with .params (oracle layout), .datas, .labs, .Ts, .max_act (and .dims, .TL, .plan, .fwd = the float64
    forward reference, .stats).  Cached: treat everything as read-only."""
    assert 0 < TL < NL
    rs = np.random.RandomState(1000003 * seed + 7919 * H + 31 * B + NL * 5 + TL)
    W, b = [], []
    W.append(rs.randint(-1, 2, size=(H, D)).astype(np.float64))
    b.append(np.full((H, 1), -2.0))
    for i in range(2, NL + 1):
        W.append(_plant_blocks(rs, _sparse_sign(rs, H, H, FF_NNZ)))
        b.append(rs.randint(-2, 3, size=(H, 1)).astype(np.float64))
    W.append(rs.randint(-1, 2, size=(A, H)).astype(np.float64))      # scaled by a power of two below
    b.append(np.zeros((A, 1)))
    Wf = _plant_blocks(rs, _sparse_sign(rs, H, H, REC_NNZ))
    Wb = _plant_blocks(rs, _sparse_sign(rs, H, H, REC_NNZ))
    Ts = _ragged_lengths(rs, B, Tmax)
    datas = [rs.randint(-3, 4, size=(D, T)).astype(np.float64) for T in Ts]
    labs = [_labels(rs, T, A) for T in Ts]
    params = {"W": W, "b": b, "Wf": Wf, "Wb": Wb}
    case = SimpleNamespace(params=params, datas=datas, labs=labs, Ts=Ts, max_act=MAX_ACT, TL=TL, NL=NL,
                           dims=(D, A, H, NL, TL, Tmax), plan=plan(Ts), seed=seed)
    # the output layer: integer x 2^-k, k from the integer logits' spread (standard deviation of order 1)
    fwd = _forward(case, None)
    k = int(np.round(np.log2(max(fwd["logits"].std(), 1.0))))
    assert 0 <= k <= 14, k                       # 2^-k is a normal float16
    W[NL] = W[NL] * 2.0 ** -k
    case.out_shift = k
    case.fwd = _forward(case, None)
    for m in W + b + [Wf, Wb] + datas:
        m.setflags(write=False)
    case.stats = _check_conditions(case)
    return case


def _check_conditions(case):
    """the conditions that keep a case from being vacuous, on the float64 reference alone; returns the shares"""
    f, pl, p = case.fwd, case.plan, case.params
    NL, TL, mx = case.NL, case.TL, case.max_act
    H = case.dims[2]
    for m in [p["Wf"], p["Wb"]] + p["W"][:NL] + p["b"][:NL] + case.datas:
        assert np.array_equal(m, np.round(m))
    assert mx == round(mx)
    assert np.array_equal(p["W"][NL] * 2.0 ** case.out_shift, np.round(p["W"][NL] * 2.0 ** case.out_shift))
    assert len(empty_blocks(p["Wf"])) == 0 and len(empty_blocks(p["Wb"])) == 0
    assert min(case.Ts) >= 1 and max(case.Ts) == case.dims[5]
    if pl.B >= 3:
        assert sum(t == 1 for t in case.Ts) >= 1 and sum(t == pl.Tmax for t in case.Ts) >= 2
        assert case.Ts != sorted(case.Ts, reverse=True)
    # integers below 2^22 in every hidden layer; what enters a 16-bit product <= 2048; recurrent state <= maxAct
    for m in f["pre"][1:NL + 1] + f["acts"][:NL + 1] + [f["preF"], f["preB"]]:
        assert np.array_equal(m, np.round(m)) and np.abs(m).max() < 2 ** 22
    for m in f["acts"][:NL + 1]:
        assert np.abs(m).max() <= 2048
    assert 0 <= f["hF"].min() and f["hF"].max() <= mx and 0 <= f["hB"].min() and f["hB"].max() <= mx
    assert np.abs(f["logits"] * 2.0 ** case.out_shift).max() < 2 ** 22
    assert 0.3 < f["logits"].std() < 3.0, f["logits"].std()
    stats = {"frames": pl.N, "max_pre": float(max(np.abs(f["preF"]).max(), np.abs(f["preB"]).max())),
             "logit_std": float(f["logits"].std())}
    t_of = np.concatenate([np.full(n, t) for t, n in enumerate(pl.nact)])
    T_of = np.empty(pl.N, dtype=np.int64)
    for b_, c in enumerate(pl.cols):
        T_of[c] = case.Ts[b_]
    for name, pre, rec in (("F", f["preF"], t_of >= 1), ("B", f["preB"], t_of <= T_of - 2)):
        is0, ismx = pre <= 0, pre >= mx
        opn = ~is0 & ~ismx
        s = {"open": float(opn.mean()), "zero": float(is0.mean()), "clipped": float(ismx.mean()),
             "units_open_once": float(opn.any(axis=1).mean()),
             "pre_eq_0": int((pre[:, rec] == 0).sum()), "pre_eq_max": int((pre[:, rec] == mx).sum())}
        assert s["open"] >= 0.05 and s["zero"] >= 0.10 and s["clipped"] >= 0.10, (name, s)
        if pl.N >= 40:
            assert s["units_open_once"] >= 0.99, (name, s)
            assert s["pre_eq_0"] >= 8 and s["pre_eq_max"] >= 8, (name, s)
        stats[name] = s
    # no utterance skipped by the oracle's CTC
    costs, _, skips = _ctc(case, f)
    assert not any(skips) and np.isfinite(costs).all()
    assert H == p["Wf"].shape[0]
    return stats


# ------------------------------------------------------------------ batched reference

def _clip(x, mx):
    return np.minimum(np.maximum(x, 0.0), mx)


def _forward(case, mutant):
    """packed float64 forward pass.  `mutant`: None, or (name, argument) -- a deliberately wrong restatement, for the
    mutation check of tests/test_exact_net_cpu.py"""
    p, pl, TL, NL = case.params, case.plan, case.TL, case.NL
    name, arg = mutant if mutant else (None, None)
    mx = arg if name == "max_act" else case.max_act
    Wf, Wb = p["Wf"], p["Wb"]
    if name in ("drop_wf", "drop_wb"):
        r0, c0 = arg                                  # one 32-column chunk dropped for one 16-row block
        Wm = np.array(Wf if name == "drop_wf" else Wb)
        Wm[r0:r0 + 16, c0:c0 + 32] = 0.0
        Wf, Wb = (Wm, Wb) if name == "drop_wf" else (Wf, Wm)
    rb, nact, Tmax = pl.rowbase, pl.nact, pl.Tmax
    acts = [_pack(case.datas, pl, case.dims[0])]
    pre = [None]
    out = {}
    for i in range(1, NL + 2):
        z = p["W"][i - 1] @ acts[i - 1] + p["b"][i - 1]
        pre.append(z)
        if i == TL:
            preF, preB = np.array(z), np.array(z)
            hF, hB = np.zeros_like(z), np.zeros_like(z)
            hF[:, :nact[0]] = _clip(z[:, :nact[0]], mx)
            for t in range(1, Tmax):
                n = nact[t]
                src = t - 2 if (name == "stale_h" and t == arg) else t - 1      # mutant: h_{t-2} at one step
                preF[:, rb[t]:rb[t] + n] += Wf @ hF[:, rb[src]:rb[src] + n]
                hF[:, rb[t]:rb[t] + n] = _clip(preF[:, rb[t]:rb[t] + n], mx)
            for u in range(Tmax - 1, -1, -1):
                n = nact[u]
                n1 = nact[u + 1] if u + 1 < Tmax else 0       # utterances with a frame u + 1: a prefix of the n
                if n1:
                    preB[:, rb[u]:rb[u] + n1] += Wb @ hB[:, rb[u + 1]:rb[u + 1] + n1]
                hB[:, rb[u]:rb[u] + n] = _clip(preB[:, rb[u]:rb[u] + n], mx)
            if name == "back_start":
                # mutant: the backward direction of caller utterance `arg` starts at Tmax - 1 instead of its own
                # T_b - 1, over the frames the longest utterance has there
                c, c0 = pl.cols[arg], pl.cols[pl.order[0]]
                zz = np.concatenate([z[:, c], z[:, c0[len(c):]]], axis=1)
                h = np.zeros(z.shape[0])
                for u in range(Tmax - 1, -1, -1):
                    pu = zz[:, u] + (Wb @ h if u < Tmax - 1 else 0.0)
                    h = _clip(pu, mx)
                    if u < len(c):
                        preB[:, c[u]], hB[:, c[u]] = pu, h
            if name == "swap_rows":
                # mutant: the rows of two utterances of equal length written to each other's place
                ca, cb = pl.cols[arg[0]], pl.cols[arg[1]]
                for m in (hF, hB):
                    m[:, ca], m[:, cb] = np.array(m[:, cb]), np.array(m[:, ca])
            out.update(z=z, preF=preF, preB=preB, hF=hF, hB=hB)
            acts.append(hF + hB)
        elif i <= NL:
            acts.append(np.maximum(z, 0.0))
        else:
            acts.append(z)
    out.update(acts=acts, pre=pre, logits=acts[-1])
    return out


def _ctc(case, fwd):
    """oracle.ctc on every utterance's softmax: (costs, packed delta (A, N), skips), caller's order"""
    pl = case.plan
    costs, skips = np.zeros(pl.B), np.zeros(pl.B, dtype=bool)
    delta = np.zeros_like(fwd["logits"])
    for b in range(pl.B):
        probs = obrnn.softmax_cols(fwd["logits"][:, pl.cols[b]])
        c, d, s = octc.ctc_loss(np.asfortranarray(probs), np.ascontiguousarray(case.labs[b], dtype=np.int32), 0)
        costs[b], skips[b] = c, bool(s)
        if not s:
            delta[:, pl.cols[b]] = d
    return costs, delta, skips


class Rounding(collections.namedtuple("Rounding", "rec16 delta state16 db16 skip")):
    """Where the backward pass of the fp16-operand configuration (NNet(fp16=True), SCTC_F16) rounds, read off run_backward
    (csrc/brnn_engine.hip), add16_kernel / cvt16_kernel (csrc/elementwise.hip) and brnn_recurrent_mh_kernel
    (csrc/recurrent.hip).  Every rounding is to nearest even; every product is exact; sums are in the accumulation type.

    Always:  every delta matrix a GEMM reads -- dlogits, the ReLU-masked output of a delta GEMM, deltasFor + deltasBack
             (summed in the accumulation type first), deltasFor and deltasBack themselves -- is read through ONE bfloat16
             shadow, by the weight gradient (A operand), by the next delta GEMM (A operand) and by the bias gradient, which
             is that GEMM's column sum of its A operand; the B operands are bfloat16 too: hActs[i], hActsFor / hActsBack,
             W^T.
    rec16    the BPTT recurrence keeps its state, its additive term (the temporal layer's delta, straight from the delta
             GEMM's accumulator) and its result in the accumulation type; with the 16-bit exchange kernel (6..16
             utterances) the state it READS from the previous step and the stationary W^T are bfloat16, with every other
             recurrent kernel they are not rounded.
    The remaining fields are what a correct device does; tests/test_exact_net_cpu.py changes one at a time:
    delta    "bf16" | "trunc" (bfloat16 by truncation) | "f16" (float16 shadows of the deltas: 5 exponent bits)
    state16  the BPTT state itself stored rounded        db16   bias gradients summed from the shadow (else: unrounded)
    skip     one operand of one GEMM left unrounded: ("dW", i, "A" | "B"), ("dgrad", i, "A"), ("dWf" | "dWb", "A")"""
    __slots__ = ()

    def __new__(cls, rec16, delta="bf16", state16=False, db16=True, skip=None):
        return super().__new__(cls, bool(rec16), delta, state16, db16, skip)


def trunc_bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64).reshape(np.shape(x))


# backward mutants that are a changed Rounding record: name -> fields (rec16 is flipped by "rec_flip")
_ROUNDING_MUTANTS = {"trunc": {"delta": "trunc"}, "f16_shadow": {"delta": "f16"}, "state16": {"state16": True},
                     "db_unrounded": {"db16": False}}


def _mutated(mixed, name, arg):
    if mixed is None or name is None:
        return mixed
    if name == "rec_flip":
        return mixed._replace(rec16=not mixed.rec16)
    if name == "unrounded":
        return mixed._replace(skip=arg)
    return mixed._replace(**_ROUNDING_MUTANTS.get(name, {}))


def pair_rows(pl, shifted=None):
    """(lo, hi): the packed rows of frames (t - 1, t) of every utterance, t = 1 .. T_b - 1, in the engine's order.  shifted
    (a mutant): caller utterance whose pairs are taken one frame late, (t, t + 1), by the same index arithmetic -- past its
    own last frame that is the row of whoever is packed there"""
    rb, nact, Tmax = pl.rowbase, pl.nact, pl.Tmax
    hi = np.concatenate([rb[t] + np.arange(nact[t]) for t in range(1, Tmax)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    lo = np.concatenate([rb[t - 1] + np.arange(nact[t]) for t in range(1, Tmax)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    if shifted is not None:
        r, T = pl.rank[shifted], pl.Ts[shifted]
        assert T > 1
        sel = np.concatenate([(np.arange(nact[t]) == r) for t in range(1, Tmax)])
        assert sel.sum() == T - 1
        lo[sel] = hi[sel]
        hi[sel] = np.minimum(np.array([rb[min(t + 1, Tmax - 1)] for t in range(1, T)]) + r, pl.N - 1)
    return lo, hi


def _backward(case, fwd, delta, dtype, mutant, mixed=None):
    """packed backward pass in `dtype` from the float64 forward reference and CTC delta; `mixed`: a Rounding record (the
    fp16-operand configuration: float64 is the model, float32 its noise estimate) or None (the reference's arithmetic)"""
    p, pl, TL, NL, mx = case.params, case.plan, case.TL, case.NL, case.max_act
    name, arg = mutant if mutant else (None, None)
    m = _mutated(mixed, name, arg)
    rb, nact, Tmax = pl.rowbase, pl.nact, pl.Tmax
    cast = lambda a: np.ascontiguousarray(a, dtype=dtype)
    if m is None:
        rnd = rnd_delta = lambda a: a
    else:
        rnd = lambda a: cast(obrnn.round_bf16(a))
        fn = {"bf16": obrnn.round_bf16, "trunc": trunc_bf16, "f16": obrnn.round_f16}[m.delta]
        rnd_delta = (lambda a: cast(fn(a)))
        if m.delta == "trunc":
            rnd = rnd_delta
    skip = m.skip if m is not None else None
    op_b = lambda a, where: a if where == skip else rnd(a)
    W = [cast(w) for w in p["W"]]
    acts = [cast(a) for a in fwd["acts"]]
    hF, hB = fwd["hF"], fwd["hB"]
    if name == "nonstrict_mask":                  # mutant: h >= 0 and h <= maxAct count as open
        mF, mB = cast((hF >= 0) & (hF <= mx)), cast((hB >= 0) & (hB <= mx))
    else:
        mF, mB = cast((hF > 0) & (hF < mx)), cast((hB > 0) & (hB < mx))
    dW, db = [None] * (NL + 1), [None] * (NL + 1)
    dWf = dWb = dF = dB = None
    shadows = {}
    d_in = cast(delta)
    d16 = rnd_delta(d_in)                         # the one shadow every reader of d_in takes
    op_a = lambda where: d_in if where == skip else d16
    for i in range(NL, -1, -1):
        dW[i] = op_a(("dW", i, "A")) @ op_b(acts[i], ("dW", i, "B")).T
        db[i] = (d16 if m is None or m.db16 else d_in).sum(axis=1, keepdims=True)
        if i == 0:
            break
        d_out = rnd(W[i].T) @ op_a(("dgrad", i, "A"))
        if i == TL:
            WfT, WbT = cast(p["Wf"].T), cast(p["Wb"].T)
            rec16 = m is not None and m.rec16
            if rec16:
                WfT, WbT = rnd(WfT), rnd(WbT)
            read = rnd_delta if rec16 else (lambda a: a)            # the state as the next step reads it
            store = rnd_delta if m is not None and m.state16 else None
            dF, dB = np.array(d_out), np.array(d_out)
            for u in range(Tmax - 1, -1, -1):
                n = nact[u]
                n1 = nact[u + 1] if u + 1 < Tmax else 0
                if n1 and not (name == "drop_bptt" and u == arg):   # mutant: no recurrent term at one step
                    dF[:, rb[u]:rb[u] + n1] += WfT @ read(dF[:, rb[u + 1]:rb[u + 1] + n1])
                dF[:, rb[u]:rb[u] + n] *= mF[:, rb[u]:rb[u] + n]
                if store:
                    dF[:, rb[u]:rb[u] + n] = store(dF[:, rb[u]:rb[u] + n])
            dB[:, :nact[0]] *= mB[:, :nact[0]]
            if store:
                dB[:, :nact[0]] = store(dB[:, :nact[0]])
            for t in range(1, Tmax):
                n = nact[t]
                dB[:, rb[t]:rb[t] + n] += WbT @ read(dB[:, rb[t - 1]:rb[t - 1] + n])
                dB[:, rb[t]:rb[t] + n] *= mB[:, rb[t]:rb[t] + n]
                if store:
                    dB[:, rb[t]:rb[t] + n] = store(dB[:, rb[t]:rb[t] + n])
            lo, hi = pair_rows(pl, arg if name == "pair_shift" else None)
            shadows["dF"], shadows["dB"] = rnd_delta(dF), rnd_delta(dB)
            dWf = (dF if skip == ("dWf", "A") else shadows["dF"])[:, hi] @ rnd(cast(hF[:, lo])).T
            dWb = (dB if skip == ("dWb", "A") else shadows["dB"])[:, lo] @ rnd(cast(hB[:, hi])).T
            d_out = dF + dB
        else:
            d_out = d_out * cast(fwd["acts"][i] > 0.0)
        d_in = d_out
        d16 = rnd_delta(d_in)
        shadows["d%d" % i] = d16
    return {"d1": d_in, "dF": dF, "dB": dB, "shadows": shadows, "grads": {"W": dW, "b": db, "Wf": dWf, "Wb": dWb}}


def reference(case, dtype=np.float64, backward=True, mutant=None, mixed=None):
    """-> dict, per utterance in the caller's order, (features, T) each: z, preF, preB, hF, hB, acts (list over layers
    0..NL+1 of per-utterance lists), logits, d1, dF, dB (deltasFor / deltasBack); and costs, skips, grads (the SUM over the
    utterances, oracle layout).  The forward pass is float64 always (it is exact); dtype=np.float32 runs the backward
    part in float32.  mixed: a Rounding record -- the backward pass of the fp16-operand configuration; then also
    shadows = {"dF", "dB", "d1", .. "d<NL>": per utterance}, the values of the 16-bit delta shadows."""
    pl = case.plan
    fwd = case.fwd if mutant is None else _forward(case, mutant)
    out = {k: _unpack(fwd[k], pl) for k in ("z", "preF", "preB", "hF", "hB", "logits")}
    out["acts"] = [_unpack(a, pl) for a in fwd["acts"]]
    if backward:
        costs, delta, skips = _ctc(case, fwd)
        bw = _backward(case, fwd, delta, dtype, mutant, mixed)
        out.update(costs=costs, skips=skips, d1=_unpack(bw["d1"], pl), dF=_unpack(bw["dF"], pl), dB=_unpack(bw["dB"], pl),
                   grads=bw["grads"])
        if mixed is not None:
            out["shadows"] = {k: _unpack(v, pl) for k, v in bw["shadows"].items()}
    return out


# ------------------------------------------------------------------ the comparisons of both suites

def forward_rows_differing(got, ref, names=("z", "hF", "hB")):
    """number of (utterance, frame) rows in which any of got[name][b] differs from ref[name][b] in a single bit after
    the cast to float32 (-0.0 == 0.0).  got / ref: name -> per-utterance list of (features, T)"""
    bad = 0
    for b in range(len(ref[names[0]])):
        row_bad = np.zeros(ref[names[0]][b].shape[1], dtype=bool)
        for n in names:
            g, r = np.asarray(got[n][b], dtype=np.float32), np.asarray(ref[n][b], dtype=np.float32)
            assert g.shape == r.shape, (n, b, g.shape, r.shape)
            row_bad |= (g != r).any(axis=0)
        bad += int(row_bad.sum())
    return bad


def row_errors(got, ref):
    """got / ref: per-utterance lists of (features, T).  -> (rho, n_dirty): the largest ||got - ref|| / ||ref|| over
    the frames whose reference column is not exactly zero, and the number of frames whose reference column is exactly
    zero while got's is not"""
    rho, dirty = 0.0, 0
    for g, r in zip(got, ref):
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        nr = np.linalg.norm(r, axis=0)
        err = np.linalg.norm(g - r, axis=0)
        zero = nr == 0
        dirty += int((zero & (np.abs(g).max(axis=0) != 0)).sum())
        if (~zero).any():
            rho = max(rho, float((err[~zero] / nr[~zero]).max()))
    return rho, dirty


def rel_fro(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref) / max(np.linalg.norm(ref), 1e-300))


def grad_tensors(grads):
    """oracle-layout gradient dict -> [(name, array)] in a fixed order"""
    out = []
    for i, (w, b) in enumerate(zip(grads["W"], grads["b"])):
        out += [("dW%d" % (i + 1), w), ("db%d" % (i + 1), np.asarray(b).reshape(-1))]
    return out + [("dWf", grads["Wf"]), ("dWb", grads["Wb"])]


# ------------------------------------------------------------------ the fp16-operand backward pass: statistics and bounds

FLOOR = 2.0 ** -24           # a relative error cannot be asked to be smaller: the results are stored in fp32
SHADOW_SHARE = 1e-3          # share of a bfloat16 delta shadow's elements that may differ from the float64 model's ...
REF_SHADOW_SHARE = 2e-4      # ... and what the float32 model alone stays within on every f16 row (the CPU suite asserts it)
REF_SEEDS = tuple(range(8))
SHADOWS = ("dF", "dB", "d1", "d2")


def mixed_stats(got, m64, max_act):
    """every figure the fp16-operand backward check looks at.  got / m64: shaped like reference(..., mixed=) -- grads, dF,
    dB and shadows[name] per utterance (the shadows as VALUES) -- m64 the float64 rounding model.  ->
    fro:<tensor>   relative Frobenius error per gradient tensor
    row:dF|dB|d1   largest per-frame relative error (d1: of the bfloat16 shadow against the model's shadow)
    open:dF|dB     elements behind a closed (0, maxAct) mask that are not exactly zero
    dirty:d1       frames of delta_1 that are zero in the model and not in got
    share:<shadow> share of the shadow's elements whose value differs from the model's (-0.0 == 0.0), no frame left out"""
    st = {}
    for (name, g), (_, r) in zip(grad_tensors(got["grads"]), grad_tensors(m64["grads"])):
        st["fro:" + name] = rel_fro(g, r)
    for k, hk in (("dF", "hF"), ("dB", "hB")):
        st["row:" + k] = row_errors(got[k], m64[k])[0]
        st["open:" + k] = sum(int((np.asarray(g)[~((h > 0) & (h < max_act))] != 0).sum()) for g, h in zip(got[k], m64[hk]))
    st["row:d1"], st["dirty:d1"] = row_errors(got["shadows"]["d1"], m64["shadows"]["d1"])
    for k in SHADOWS:
        pairs = [(np.asarray(g, dtype=np.float32), np.asarray(r, dtype=np.float32)) for g, r in zip(got["shadows"][k], m64["shadows"][k])]
        assert all(g.shape == r.shape for g, r in pairs) and len(pairs) == len(m64["hF"])
        st["share:" + k] = sum(int((g != r).sum()) for g, r in pairs) / float(sum(r.size for _, r in pairs))
    return st


@functools.lru_cache(maxsize=None)
def mixed_e_ref(H, B, NL, TL, Tmax, rec16):
    """per statistic: the largest over seeds 0..7 of this shape of the float32-accumulating rounding model against the
    float64-accumulating one (not floored).  Several seeds, because one rounding flip moves a figure and the device's
    flips need not be NumPy's."""
    worst = {}
    for seed in REF_SEEDS:
        case = make_case.__wrapped__(H, B, NL=NL, TL=TL, Tmax=Tmax, seed=seed)
        mixed = Rounding(rec16)
        st = mixed_stats(reference(case, np.float32, mixed=mixed), reference(case, mixed=mixed), case.max_act)
        for k, v in st.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def mixed_violations(st, e_ref, margin):
    """the rules of tests/test_gpu_recurrence_exact.py on mixed_stats' figures -> the list of those broken"""
    out = []
    for k, v in sorted(st.items()):
        kind = k.split(":")[0]
        if kind in ("fro", "row"):
            bound = margin * max(e_ref[k], FLOOR)
            if not v <= bound:
                out.append("%s %.3g > %g x max(%.3g, 2^-24)" % (k, v, margin, e_ref[k]))
        elif kind == "share":
            if not v <= SHADOW_SHARE:
                out.append("%s %.3g > %g" % (k, v, SHADOW_SHARE))
        elif v != 0:
            out.append("%s %d != 0" % (k, v))
    return out


def rounding_of(c):
    """the Rounding record of a GPU_CASES row (None: not the fp16-operand configuration)"""
    return Rounding(rec16=c.path == "mh") if c.mode == "f16" else None


# ------------------------------------------------------------------ the GPU matrix

def _c(path, H, B, variant="0", mode="f32", NL=2, TL=1, Tmax=None, rec_path=(1, 1, 0), seed=0):
    Tmax = Tmax or (16 if B <= 8 else (14 if B <= 32 else 12))
    return SimpleNamespace(path=path, H=H, B=B, variant=variant, mode=mode, NL=NL, TL=TL, Tmax=Tmax, rec_path=rec_path,
                           seed=seed,
                           id="%s-H%d-B%d-v%s-%s" % (path, H, B, variant, mode))


# path names follow rec_plan / rec_cut (csrc/recurrent_plan.h; rec_cut cuts some minibatches into two launches, noted per
# row): tests/test_recurrence_plan_cpu.py holds every row to its name.  mode: "f32" | "bf16x3" | "f16" (NNet(fp16=True)).
GPU_CASES = (
    # 1..3 utterances: sentinel / VALU kernel, 4-utterance instantiation (the flag kernel takes over at 4)
    [_c("s4", H, B) for H in (512, 1824) for B in (1, 3)]
    + [_c("s8", 1024, 7, variant="43")]
    # 4..16: the flag kernel as ONE chain per direction (half its grid)
    + [_c("q1", 512, 4), _c("q1", 1024, 11), _c("q1", 1824, 4), _c("q1", 1824, 11), _c("q1", 1824, 16), _c("q1", 2048, 16)]
    # fp16 operands, 6..16: 16-bit exchange (float16 forward, bfloat16 BPTT)
    + [_c("mh", H, B, mode="f16") for H in (512, 1824) for B in (6, 16)]
    # fp16 operands around an fp32 recurrence: sentinel kernel at 2, two-chain flag kernel at 24
    + [_c("s4", 512, 2, mode="f16"), _c("q2", 512, 24, mode="f16")]
    # fp16 operands, the rest of what a backward pass can meet: other chunk counts per wave of the 16-bit exchange kernel
    # and an odd minibatch; the single-chain flag kernel at 5; 40 utterances (one launch: no cut with 16-bit operands); the
    # per-step fallback; a ReLU layer below the temporal one (its delta GEMM masks by the sign of a 16-bit shadow)
    + [_c("mh", 1024, 12, mode="f16"), _c("mh", 2048, 9, mode="f16"), _c("q1", 512, 5, mode="f16"),
       _c("slab", 512, 40, mode="f16"), _c("fallback", 512, 7, variant="3", mode="f16", rec_path=(3, 3, 0)),
       # (12 utterances, not the fp32 row's 5: with 11 000 elements per shadow three rounding flips of the float32 model
       # would already be more than the 2e-4 the CPU suite holds it to)
       _c("below-tl", 200, 12, NL=3, TL=2, mode="f16")]
    # 17..32 at the large layers: 16 units x both tiles of a direction per CU
    + [_c("t-ug1", H, B) for H in (1824, 2048) for B in (17, 24, 32)]
    # 17..32 at the small layers, and at the large one when asked for: two chains per CU
    + [_c("q2", H, B) for H in (512, 1024) for B in (17, 32)]
    + [_c("q2", 1824, 24, variant="51")]
    # 33..128 tiled: one tile per sub-chain (<= 64), two tiles (> 64)
    + [_c("t-1tile", H, B) for H in (1824, 2048) for B in (33, 64)]
    + [_c("t-2tile", H, B) for H in (1824, 2048) for B in (100, 128)]
    # 80 utterances: 64 (tiled) + 16 (single chain) by default, one launch of the two-tile form with variant 45
    + [_c("t-cut64", 1824, 80), _c("t-nocut", 1824, 80, variant="45")]
    + [_c("t-small", H, B, variant="50") for H in (512, 1024) for B in (40, 100)]
    # one slab per CU: NTW = 1 / 2 / 4
    + [_c("slab", 512, B, variant="1") for B in (9, 40, 100)]
    # the default cut at the small layers: 32 (two chains) + 8 (single chain)
    + [_c("cut32", 512, 40)]
    # layer sizes without a specialised kernel (generic instantiation; 40 = 32 + 8 by default)
    + [_c("generic", H, B) for H in (96, 132) for B in (5, 40, 128)]
    + [_c("fallback", 512, 7, variant="3", rec_path=(3, 3, 0)), _c("fallback", 96, 20, variant="3", rec_path=(3, 3, 0))]
    # more than 128 utterances: 128 + 22
    + [_c("two-launches", 64, 150)]
    + [_c("below-tl", 200, 5, NL=3, TL=2)]
    + [_c("bf16x3", 512, 8, mode="bf16x3")]
)


def gpu_case(c):
    return make_case(c.H, c.B, NL=c.NL, TL=c.TL, Tmax=c.Tmax, seed=c.seed)
