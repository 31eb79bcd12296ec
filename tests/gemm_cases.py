"""The case table of tests/test_gpu_gemm_options.py and its host data, shared with tests/test_gemm_model_cpu.py
(which proves on the CPU that every case is exact in fp32 and sees every mutation of tests/gemm_model.py).

An implementation is one GEMM kernel family selected through environment variables the library reads on every call;
shapes are named relative to its tile (BM, BN, K tile).  Data: operands integers in [-3, 3], bias / addend / previous
C small integers, add_scale 0.25, mask values from {negative, -0.0, +0.0, smallest denormal, positive}; every
operand buffer has a padded leading dimension with NaN in the padding, in the rows past K and in the rows no gather
index names; every output buffer is sentinel-filled with padding and slack.  Seeds are fixed by the case's name.
The one deviation from "small": cases that write a 16-bit shadow AND have a bias draw that bias from +-[2100, 4000],
so that the results are not representable in float16 / bfloat16 and a wrong rounding mode shows."""
import zlib
from types import SimpleNamespace

import numpy as np

from tests import gemm_model

SENT = -12345.0          # fp32 sentinel of output buffers
SENT16 = 0x5A5A          # 16-bit sentinel
NAN16 = 0x7FFF           # NaN in float16 and in bfloat16
ADD_SCALE = 0.25

# name -> environment, GemmArgs.prec / in16, (BM, BN, K tile)
IMPLS = {
    "f32_shape0": dict(env={"SCTC_GEMM_SHAPE": "0"}, prec=0, in16=0, tile=(128, 128, 16)),
    "f32_shape1": dict(env={"SCTC_GEMM_SHAPE": "1"}, prec=0, in16=0, tile=(128, 96, 16)),
    "f32_shape2": dict(env={"SCTC_GEMM_SHAPE": "2"}, prec=0, in16=0, tile=(64, 128, 16)),
    "f32_shape3": dict(env={"SCTC_GEMM_SHAPE": "3"}, prec=0, in16=0, tile=(128, 64, 16)),
    "f16_round_tile0": dict(env={"SCTC_H16_TILE": "0"}, prec=1, in16=0, tile=(128, 128, 32)),
    "f16_round_tile1": dict(env={"SCTC_H16_TILE": "1"}, prec=1, in16=0, tile=(256, 256, 32)),
    "bf16_round_tile0": dict(env={"SCTC_H16_TILE": "0"}, prec=2, in16=0, tile=(128, 128, 32)),
    "bf16_round_tile1": dict(env={"SCTC_H16_TILE": "1"}, prec=2, in16=0, tile=(256, 256, 32)),
    "f16_mem_tile0": dict(env={"SCTC_H16_TILE": "0"}, prec=1, in16=1, tile=(128, 128, 64)),
    "bf16_mem_tile0": dict(env={"SCTC_H16_TILE": "0"}, prec=2, in16=1, tile=(128, 128, 64)),
    # the LDS-DMA kernel (K tile 32) where csrc/gemm_plan.h picks GEMM_G16, else the register-staged 256 tile (K tile 64)
    "f16_mem_tile1": dict(env={"SCTC_H16_TILE": "1"}, prec=1, in16=1, tile=(256, 256, 32)),
    "bf16_mem_tile1": dict(env={"SCTC_H16_TILE": "1"}, prec=2, in16=1, tile=(256, 256, 32)),
    "bf16x3": dict(env={"SCTC_H16_TILE": "0"}, prec=3, in16=0, tile=(128, 128, 16)),
}
ENV_NAMES = ("SCTC_GEMM_SHAPE", "SCTC_H16_TILE", "SCTC_G16")


def case_tile(c):
    """(BM, BN, K tile) of the kernel that runs case c; held against csrc/gemm_plan.h by tests/test_gemm_plan_cpu.py"""
    im = IMPLS[c.impl]
    bm, bn, bk = im["tile"]
    if im["in16"] and bm == 256:
        g16 = "gather" not in c.opts and (c.lay == "NT" or (c.M % 8 == 0 and c.N % 8 == 0))
        if not g16:
            bk = 64
    return bm, bn, bk


def _case(impl, lay, M, N, K, splits, opts, **quirks):
    opts = frozenset(opts.split())
    name = "%s-%s-%dx%dx%d-s%d-%s" % (impl, lay, M, N, K, splits, "+".join(sorted(opts)) or "plain")
    for q in sorted(quirks):
        name += "-" + q
    return SimpleNamespace(impl=impl, lay=lay, M=M, N=N, K=K, splits=splits, opts=opts, quirks=quirks, name=name)


def cases_for(impl):
    im = IMPLS[impl]
    BM, BN, BK = im["tile"]
    prec, in16 = im["prec"], im["in16"]
    kq = 8 if in16 else 4                      # K-contiguous operands: K a multiple of this
    shadows = prec in (1, 2)
    out, seen = [], set()

    def add(lay, M, N, K, splits, opts, **quirks):
        if lay != "TN":
            K = (K + kq - 1) // kq * kq
        c = _case(impl, lay, M, N, K, splits, opts, **quirks)
        if c.name not in seen:                 # the sections overlap in a few cases
            seen.add(c.name)
            out.append(c)

    FWD = "bias relu"
    FWD16 = "bias relu c16a c16b skip"
    WG = "colsum addend"
    RWG = "gather acc addend"
    delta_lay = "NT" if in16 else "NN"
    shapes = [(4, 4, 4), (BM, BN, BK), (BM + 4, BN + 4, BK + 4), (3 * BM, 3 * BN, 4 * BK + 4)]
    # ---- every shape with the option sets the engine issues
    for i, (M, N, K) in enumerate(shapes):
        add("NT", M, N, K, (1, 1, 2, 3)[i], FWD)
        add(delta_lay, M, N, K, 1, "mask")
        add("TN", M, N, K, (1, 1, 2, 4)[i], WG + " acc")
        add("TN", M, N, K, (1, 2, 3, 3)[i], WG)
        if not in16:
            add("TT", M, N, K, 1, "bias")
        if shadows:
            add("NT", M, N, K, 1, FWD16)
            add(delta_lay, M, N, K, 1, "mask16 c16b skip")
            add(delta_lay, M, N, K, 1, "mask16 c16b skip bias")
        if i >= 2:
            add("TN", M, N, K, (1, 3)[i - 2], RWG)
            if prec == 0:
                add("NT", M, N, K, (2, 3)[i - 2], FWD + " a2 asum")
                add("TN", M, N, K, (1, 4)[i - 2], WG + " acc a2 asum")
    # ---- each option alone, two tiles in each direction with a ragged edge
    M, N, K = shapes[2]
    for o in ("", "bias", "relu", "mask", "addend", "acc"):
        add("NT", M, N, K, 1, o)
    add("NT", M, N, K, 1, "colsum")                  # K-contiguous A: the column sums must stay untouched
    add("NT", M, N, K, 2, "colsum")
    add("TN", M, N, K, 1, "colsum")
    add("TN", M, N, K, 1, "gather")
    if prec != 0:
        add("NT", M, N, K, 1, "mask16")
    if prec == 0:
        add("NT", M, N, K, 1, "a2")
        add("TN", M, N, K, 1, "a2 asum")
    if shadows:
        add("NT", M, N, K, 1, "c16a")
        add("NT", M, N, K, 1, "c16b")
        add("NT", M, N, K, 1, "c16a skip")
    # the order of the epilogue steps
    add("NT", M, N, K, 1, "bias relu mask addend acc")
    add("NT", M, N, K, 3, "bias relu mask addend acc")
    if prec != 0:
        add("NT", M, N, K, 1, "bias mask16 addend")
    # ---- split-K: 5 K tiles, the last one ragged; 3 leaves the last slice one K tile, 4 leaves it none
    for s in (1, 2, 3, 4):
        add("NT", M, N, 4 * BK + 4, s, FWD)
        add("TN", M, N, 4 * BK + 4, s, WG)
        add("TN", M, N, 4 * BK + 4, s, RWG)
        if shadows and s > 1:                       # the reduce kernel then applies the epilogue and writes the shadows
            add("NT", M, N, 4 * BK + 4, s, FWD16)
            add(delta_lay, M, N, 4 * BK + 4, s, "mask16 c16b skip")
    # ---- K edges in the row-contiguous / row-contiguous layout; K = 0 still applies bias, addend, accumulate
    for K_, s in ((0, 1), (0, 2), (1, 1), (17, 1), (17, 2), (2 * BK + 1, 1), (2 * BK + 1, 2), (2 * BK + 1, 3)):
        add("TN", M, N, K_, s, "bias addend acc colsum")
    add("TN", M, N, 0, 1, "bias addend colsum")       # K = 0 without accumulate: the column sums become zero
    add("TN", M, N, 0, 2, "colsum")
    # ---- the scalar epilogue
    if impl == "f32_shape0" or prec != 0:
        sc = "bias relu mask addend acc" + (" c16a" if shadows else "")
        for N_ in (33, BN + 1):
            add("NT", M, N_, K, 1, sc)
            add("NT", M, N_, 4 * BK + 4, 2, sc)
        for quirk in ("odd_ldc", "odd_ldmask", "odd_ldadd"):
            add("NT", M, N, K, 1, "bias mask addend acc", **{quirk: 1})
        add("NT", M, N, K, 1, FWD, bias_off=1)
    # ---- the LDS-DMA kernel's row-contiguous layout: M and N multiples of 8, not of its tile
    if in16 and BM == 256:
        for s in (1, 3, 4):
            add("TN", 264, 136, 4 * BK + 4, s, WG + " acc")
    # ---- a shape the planner splits by itself, with the planner's own count and workspace
    add("TN", M, N, 2052, 0, WG + " planner")
    if prec == 0:
        add("TN", M, N, 1296, 10, WG)             # 81 K tiles of 16 in 10 slices of 9: the last one is empty
    return out


def _ints(rs, shape, lo, hi):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)


def _reals(rs, shape, lo, hi):
    """the non-integer pass: standard normal values whatever the integer range"""
    return rs.standard_normal(size=shape).astype(np.float32)


def _operand(rs, rows, K, kcontig, in16, gather, draw):
    """image of an operand standing for a rows x K matrix; returns (image, idx or None)"""
    al = 8 if in16 else 4
    if kcontig:
        ld = (K + al - 1) // al * al + al
        img = np.full((rows, ld), np.nan, dtype=np.float32)
        img[:, :K] = draw(rs, (rows, K), -3, 3)
        return img, None
    ld = (rows + al - 1) // al * al + al
    R = K + (7 if gather else 3)
    img = np.full((R, ld), np.nan, dtype=np.float32)
    if not gather:
        img[:K, :rows] = draw(rs, (K, rows), -3, 3)
        return img, None
    named = np.sort(rs.choice(R - 1, size=max(1, R - 4), replace=False))    # row R - 1 is never named
    img[named, :rows] = draw(rs, (len(named), rows), -3, 3)
    idx = rs.choice(named, size=K)                      # repeats
    h = K // 2
    idx[:h] = np.sort(idx[:h])[::-1]                    # a descending run
    return img, idx.astype(np.int32)


def _mask_pick(rs, M, N):
    """which of the five mask values goes where: random, but a tiny matrix gets every value several times"""
    if M * N >= 256:
        return rs.randint(0, 5, size=(M, N))
    return (3 * np.arange(M)[:, None] + np.arange(N)[None, :] + rs.randint(5)) % 5


def host_data(c, real=False):
    """everything a launch of case c reads, and the initial images of everything it may write.  real: the
    non-integer pass (standard normal data; 16-bit operands in memory rounded to their type)"""
    im = IMPLS[c.impl]
    ints = _reals if real else _ints
    draw = ints
    if real and im["in16"]:
        rnd = gemm_model.round_f16 if im["prec"] == 1 else gemm_model.round_bf16
        draw = lambda rs_, shape, lo, hi: rnd(_reals(rs_, shape, lo, hi)).astype(np.float32)     # noqa: E731
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    o, M, N, K = c.opts, c.M, c.N, c.K
    akc, bkc = int(c.lay[0] == "N"), int(c.lay[1] == "T")
    d = SimpleNamespace(akc=akc, bkc=bkc, prec=im["prec"], in16=im["in16"])
    gather = "gather" in o
    d.A, d.idx_a = _operand(rs, M, K, akc, d.in16, gather and not akc, draw)
    d.B, d.idx_b = _operand(rs, N, K, bkc, d.in16, gather and not bkc, draw)
    d.A2 = None
    if "a2" in o:
        d.A2 = d.A.copy()
        live = ~np.isnan(d.A)
        d.A2[live] = draw(rs, int(live.sum()), -3, 3)
    big_bias = "bias" in o and ("c16a" in o or "c16b" in o) and not real
    d.bias_off = int(c.quirks.get("bias_off", 0))
    d.bias_buf = None
    if "bias" in o:
        d.bias_buf = np.full(N + 4, np.nan, dtype=np.float32)
        b = ints(rs, N, 2100, 4000) * rs.choice([-1.0, 1.0], size=N).astype(np.float32) if big_bias else ints(rs, N, -8, 8)
        d.bias_buf[d.bias_off:d.bias_off + N] = b
    n4 = (N + 3) // 4 * 4
    d.ldc = n4 + 4 + int(c.quirks.get("odd_ldc", 0))
    d.C0 = np.full((M + 1, d.ldc), SENT, dtype=np.float32)            # one row of slack
    if "acc" in o:
        d.C0[:M, :N] = ints(rs, (M, N), -8, 8)
    d.mask = d.mask16 = d.addend = None
    if "mask" in o:
        d.mask = np.full((M, n4 + 4 + int(c.quirks.get("odd_ldmask", 0))), np.nan, dtype=np.float32)
        vals = np.array([-1.5, -0.0, 0.0, np.float32(1e-45), 2.0], dtype=np.float32)
        d.mask[:, :N] = vals[_mask_pick(rs, M, N)]
        if real:
            d.mask[:, :N] = _reals(rs, (M, N), 0, 0)
    if "mask16" in o:
        d.mask16 = np.full((M, n4 + 4), NAN16, dtype=np.uint16)
        vals = np.array([0xBC00, 0x8000, 0x0000, 0x0001, 0x3C00], dtype=np.uint16)
        d.mask16[:, :N] = vals[_mask_pick(rs, M, N)]
    if "addend" in o:
        d.addend = np.full((M, n4 + 4 + int(c.quirks.get("odd_ldadd", 0))), np.nan, dtype=np.float32)
        d.addend[:, :N] = ints(rs, (M, N), -8, 8)
    d.ldc16 = n4 + 4
    d.C16a0 = np.full((M + 1, d.ldc16), SENT16, dtype=np.uint16) if "c16a" in o else None
    d.C16b0 = np.full((M + 1, d.ldc16), SENT16, dtype=np.uint16) if "c16b" in o else None
    d.colsum0 = None
    if "colsum" in o:
        d.colsum0 = np.full(M + 5, SENT, dtype=np.float32)
        if "acc" in o:
            d.colsum0[:M] = ints(rs, M, -8, 8)
    d.asum0 = np.full(d.A.shape, SENT, dtype=np.float32) if "asum" in o else None
    return d


def model_args(c, d, splits=None):
    o = c.opts
    return gemm_model.args(
        A=d.A, B=d.B, C=d.C0, M=c.M, N=c.N, K=c.K, a_kcontig=d.akc, b_kcontig=d.bkc, idx_a=d.idx_a, idx_b=d.idx_b,
        bias=None if d.bias_buf is None else d.bias_buf[d.bias_off:d.bias_off + c.N], mask=d.mask, addend=d.addend,
        add_scale=ADD_SCALE, relu=int("relu" in o), accumulate=int("acc" in o), colsum_a=d.colsum0,
        splits=c.splits if splits is None else splits, prec=d.prec, in16=d.in16, C16a=d.C16a0, C16b=d.C16b0,
        skip_c32=int("skip" in o), mask16=d.mask16, A2=d.A2, a_sum=d.asum0)


def expected_images(c, d, out):
    """the full images (padding, slack and sentinels included) of every output buffer after the launch"""
    M, N, K = c.M, c.N, c.K
    e = SimpleNamespace(C=d.C0.copy(), C16a=None, C16b=None, colsum=None, asum=None)
    if out.C is not None:
        e.C[:M, :N] = out.C.astype(np.float32)
    for nm, init in (("C16a", d.C16a0), ("C16b", d.C16b0)):
        if init is not None:
            img = init.copy()
            if getattr(out, nm) is not None:
                img[:M, :N] = getattr(out, nm)
            setattr(e, nm, img)
    if d.colsum0 is not None:
        e.colsum = d.colsum0.copy()
        if out.colsum_a is not None:
            e.colsum[:M] = out.colsum_a.astype(np.float32)
    if d.asum0 is not None:
        e.asum = d.asum0.copy()
        if out.a_sum is not None:
            if d.akc:
                e.asum[:M, :K] = out.a_sum.astype(np.float32)
            else:
                e.asum[:K, :M] = out.a_sum.astype(np.float32)
    return e


def applicable_mutations(c, splits=None):
    """the mutations of gemm_model.MUTATIONS case c must notice"""
    o, M, N, K = c.opts, c.M, c.N, c.K
    BM, BN, BK = case_tile(c)
    s = c.splits if splits is None else splits
    tn_colsum = "colsum" in o and c.lay[0] == "T"
    masked = "mask" in o or "mask16" in o
    m = []
    if K > 0:
        m.append("drop_last_k")
    if tn_colsum and s > 1:
        ktiles = (K + BK - 1) // BK
        per = (ktiles + s - 1) // s
        if (s - 1) * per * BK < K:
            m.append("colsum_drop_last_slice")
    if tn_colsum and N > BN and K > 0:
        m.append("colsum_every_n_tile")
    if "acc" in o:
        m.append("ignore_accumulate_c")
        if tn_colsum:
            m.append("ignore_accumulate_colsum")
    if masked:
        m += ["mask_negzero_positive", "mask_poszero_positive"]
        if "bias" in o:
            m.append("mask_first")
        if "addend" in o:
            m.append("mask_last")
        if M > 1:
            m.append("mask_shift_row")
        if N > 4:
            m.append("mask_shift_group")
    if "addend" in o:
        if M > 1:
            m.append("addend_shift_row")
        if N > 4:
            m.append("addend_shift_group")
    if "gather" in o and K > 0:
        m += ["gather_shift_one", "swap_idx"]
    if "a2" in o and K > 0:
        m.append("a2_not_in_product")
    if "asum" in o and K > 0:
        m.append("a2_not_in_asum")
        if M > BN:
            m.append("asum_first_tile_rows_only")
    if ("c16a" in o or "c16b" in o) and "bias" in o:
        m.append("shadow_round_to_zero")
    if "skip" in o:
        m.append("write_c_despite_skip")
    return m
