"""float64 NumPy restatement of one launch_gemm_f32(GemmArgs) call (stanford-ctc_amd/csrc/gemm_f32.h), written
from that header's comments, not from the kernels:

    C[M][N] = sum_k A(m,k) B(k,n), then   acc (+ bias[n]) -> relu -> mask / mask16 -> + add_scale * addend -> (+ C_prev)

    A(m,k) = A[m][k] when a_kcontig, else A[ka(k)][m], ka(k) = idx_a ? idx_a[k] : k        (B alike, with n)
    A2      : A(m,k) = fp32(A[..] + A2[..]);  a_sum (same layout as A) receives that sum over the logical M x K region
    mask    : keep where the fp32 value is > 0;  mask16: keep where the sign bit is clear and the other 15 bits nonzero
    colsum_a[m] (+)= sum_k A(m,k), only for a row-contiguous A, `accumulate` selects += like for C; of the sum
              A + A2, of the 16-bit values with in16, of the UNROUNDED fp32 values with prec 1 / 2 on fp32 operands
    prec 1 / 2 on fp32 operands: both operands rounded (nearest even) to float16 / bfloat16 for the product
    C16a / C16b : the fp32 result rounded to nearest even to float16 / bfloat16;  skip_c32: C itself is not written

`gemm_model` takes the operands as the host images of the device buffers (2-D arrays, padding included) and returns
what a launch may write -- the LOGICAL regions only: C, C16a, C16b, colsum_a, a_sum; None = "this launch does not
touch it".  `mut` names one deliberate mistake (MUTATIONS): tests/test_gemm_model_cpu.py proves that every case of the
GPU table would notice each of them, so a kernel making that mistake cannot pass tests/test_gpu_gemm_options.py."""
from types import SimpleNamespace

import numpy as np

from oracle.brnn import round_bf16, round_f16     # noqa: F401  operand rounding: the oracle's (nearest even)

MUTATIONS = (
    "drop_last_k",              # the K tail: the last K element never multiplied (nor summed)
    "colsum_drop_last_slice",   # the column sums miss the K rows of the last split-K slice
    "colsum_every_n_tile",      # every N tile adds its column sums instead of the first one only
    "ignore_accumulate_c", "ignore_accumulate_colsum",
    "mask_first", "mask_last",  # mask applied before bias and relu / after the addend
    "mask_shift_row", "mask_shift_group", "addend_shift_row", "addend_shift_group",   # one row / one 4-column group off
    "mask_negzero_positive", "mask_poszero_positive",
    "gather_shift_one", "swap_idx",
    "a2_not_in_product", "a2_not_in_asum", "asum_first_tile_rows_only",
    "shadow_round_to_zero", "write_c_despite_skip",
)


def args(**kw):
    """a GemmArgs-like namespace: every field of the struct, null / zero by default"""
    d = dict(A=None, B=None, C=None, M=0, N=0, K=0, a_kcontig=1, b_kcontig=1, idx_a=None, idx_b=None, bias=None,
             mask=None, addend=None, add_scale=0.0, relu=0, accumulate=0, colsum_a=None, splits=1, prec=0, in16=0,
             C16a=None, C16b=None, skip_c32=0, mask16=None, A2=None, a_sum=None)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    return SimpleNamespace(**d)


def f16_bits(x, toward_zero=False):
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = x.astype(np.float16)
    bits = h.view(np.uint16).copy()
    if toward_zero:         # nearest-even went away from zero: one step back (sign-magnitude bits)
        bits[np.abs(h.astype(np.float32)) > np.abs(x)] -= 1
    return bits


def bf16_bits(x, toward_zero=False):
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    if toward_zero:
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def pos16(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return ((bits & 0x8000) == 0) & ((bits & 0x7FFF) != 0)


def _logical(mem, kcontig, idx, rows, K):
    """the rows x K matrix X(r, k) an operand image stands for"""
    if kcontig:
        return np.asarray(mem)[:rows, :K]
    ks = np.arange(K) if idx is None else np.asarray(idx)[:K]
    return np.asarray(mem)[ks, :rows].T


def _shift(x, rows=0, cols=0):
    """x read `rows` rows / `cols` columns further on (cyclic: stays inside the logical region)"""
    return np.roll(np.roll(x, -rows, axis=0), -cols, axis=1)


def gemm_model(g, mut=None, tile=(128, 128, 16)):
    """g: args(...).  tile = (BM, BN, K tile) of the implementation, used by the mutations only."""
    assert mut is None or mut in MUTATIONS, mut
    M, N, K = g.M, g.N, g.K
    BM, BN, BKT = tile
    idx_a, idx_b = g.idx_a, g.idx_b
    if mut == "swap_idx":
        idx_a, idx_b = idx_b, idx_a
    if mut == "gather_shift_one":
        idx_a = np.array(idx_a).copy()
        idx_a[K // 2] += 1
    A32 = _logical(g.A, g.a_kcontig, idx_a, M, K).astype(np.float32)
    Asum32 = A32
    if g.A2 is not None:
        Asum32 = A32 + _logical(g.A2, g.a_kcontig, idx_a, M, K).astype(np.float32)     # ONE fp32 add
    Aprod = A32 if mut == "a2_not_in_product" else Asum32
    Bprod = _logical(g.B, g.b_kcontig, idx_b, N, K).astype(np.float32)
    Kp = K - 1 if (mut == "drop_last_k" and K > 0) else K
    if g.prec in (1, 2) and not g.in16:
        rnd = round_f16 if g.prec == 1 else round_bf16
        Ap, Bp = rnd(Aprod), rnd(Bprod)
    else:
        Ap, Bp = Aprod.astype(np.float64), Bprod.astype(np.float64)
    acc = Ap[:, :Kp] @ Bp[:, :Kp].T

    def keep_mask():
        if g.mask is not None:
            m = np.asarray(g.mask)[:M, :N].astype(np.float32)
            keep = m > 0
            if mut == "mask_negzero_positive":
                keep = keep | ((m == 0) & np.signbit(m))
            if mut == "mask_poszero_positive":
                keep = keep | ((m == 0) & ~np.signbit(m))
        else:
            m = np.asarray(g.mask16)[:M, :N]
            keep = pos16(m)
            if mut == "mask_negzero_positive":
                keep = keep | (m == 0x8000)
            if mut == "mask_poszero_positive":
                keep = keep | (m == 0)
        if mut == "mask_shift_row":
            keep = _shift(keep, rows=1)
        if mut == "mask_shift_group":
            keep = _shift(keep, cols=4)
        return keep

    has_mask = g.mask is not None or g.mask16 is not None
    v = acc
    if has_mask and mut == "mask_first":
        v = np.where(keep_mask(), v, 0.0)
    if g.bias is not None:
        v = v + np.asarray(g.bias, dtype=np.float64)[None, :N]
    if g.relu:
        v = np.maximum(v, 0.0)
    if has_mask and mut not in ("mask_first", "mask_last"):
        v = np.where(keep_mask(), v, 0.0)
    if g.addend is not None:
        add = np.asarray(g.addend)[:M, :N].astype(np.float64)
        if mut == "addend_shift_row":
            add = _shift(add, rows=1)
        if mut == "addend_shift_group":
            add = _shift(add, cols=4)
        v = v + float(np.float32(g.add_scale)) * add
    if has_mask and mut == "mask_last":
        v = np.where(keep_mask(), v, 0.0)
    if g.accumulate and mut != "ignore_accumulate_c":
        v = v + np.asarray(g.C)[:M, :N].astype(np.float64)

    out = SimpleNamespace(C=None, C16a=None, C16b=None, colsum_a=None, a_sum=None)
    if not g.skip_c32 or mut == "write_c_despite_skip":
        out.C = v
    v32 = v.astype(np.float32)
    rtz = mut == "shadow_round_to_zero"
    if g.C16a is not None:
        out.C16a = f16_bits(v32, rtz)
    if g.C16b is not None:
        out.C16b = bf16_bits(v32, rtz)

    if g.colsum_a is not None and not g.a_kcontig:
        ks = Kp
        if mut == "colsum_drop_last_slice" and g.splits > 1:
            ktiles = (K + BKT - 1) // BKT
            per = (ktiles + g.splits - 1) // g.splits
            ks = min(K, (g.splits - 1) * per * BKT)
        cs = Asum32.astype(np.float64)[:, :ks].sum(axis=1)
        if mut == "colsum_every_n_tile":
            cs = cs * ((N + BN - 1) // BN)
        if g.accumulate and mut != "ignore_accumulate_colsum":
            cs = cs + np.asarray(g.colsum_a, dtype=np.float64)[:M]
        out.colsum_a = cs
    if g.a_sum is not None and g.A2 is not None:
        s = A32 if mut == "a2_not_in_asum" else Asum32           # [M][K]
        s = s.astype(np.float64)
        if mut == "asum_first_tile_rows_only":
            s = s.copy()
            s[BN:, :] = np.nan                                   # "never stored"
        out.a_sum = s if g.a_kcontig else s.T                    # the layout of A: [M][K] or [K][M]
    return out
