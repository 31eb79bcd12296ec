// fp32-accurate GEMM on the bfloat16 matrix cores (GemmArgs::prec == 3, SCTC_BF16X3): the same
// contractions as gemm_f32.hip (brnnet.py:140 fwd, :196 wgrad, :204 dgrad, :227-230 recurrent wgrad).
//
// Every fp32 operand element is split EXACTLY into three bfloat16 terms, x = x1 + x2 + x3
// (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2): 3 x 8 significand bits, the subtractions
// are exact), and six of the nine cross products run on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation: x1y1, x1y2, x2y1, x2y2, x1y3, x3y1.  The dropped x2y3 + x3y2 + x3y3 are below
// 2^-23 |xy|, the same size as ONE fp32 rounding of the product; measured against a float64 product
// the error equals that of the fp32 fma chain of gemm_f32.hip (tests/test_gpu_bf16x3.py,
// tests/gpu_diag.py gemmx3).  Six bfloat16 MFMAs cost 6/16 of the fp32 MFMA time for the same tile.
// Caveat: an Inf / NaN operand element turns its whole product row into NaN (Inf - Inf in the split).
//
// Kernel: 128x128 tile, 256 threads = 2x2 waves of 64x64, K tile 16, two blocks per CU (LDS: two
// buffers x 6 planes x 128 rows x 48 B = 72 KiB per block).  A wave issues in order, so one K tile is a
// software pipeline inside the instruction stream, written as 24 slots of [one MFMA + a piece of the
// other work] fenced with sched_barrier: while the 24 MFMAs of tile t run (24 x 32 matrix-core
// cycles) the same wave splits tile t+1 -- fetched FOUR tiles earlier into one of four rotating
// register sets; with one set (one tile of slack) the step time WAS the memory latency -- into the
// other LDS buffer and requests tile t+5.  The second block of the CU fills the fragment-read and
// barrier gaps.  History (64000 x 2048 x 2048, fp32 kernel 4.4 ms): un-pipelined, 2 blocks per CU, one
// LDS buffer 3.45 ms = 2.11 ms without the MFMAs + 1.29 ms of ideal MFMA time, i.e. fully serialised;
// K tile 32 pipelined with one register set, one block per CU 2.93 ms; this kernel 2.81 ms = 191 TFLOP/s.
// s_memtime stamps (-DSCTC_S3_STAMP, tests/gpu_diag.py s3stamp): forward (NT) 2030 shader cycles per step
// of the two resident blocks against 1536 of matrix-core time -- 76 % busy -- at a shader clock of 1.44 GHz:
// the kernel is POWER-bound (a register-only loop of this MFMA on random operands sustains 1775 TFLOP/s =
// 1.7 GHz, tools/valu_rate.hip; with the split's VALU and LDS traffic on top the clock drops further).
// Two things that were worth more than any schedule (weight gradient 122 -> 162, delta propagation 157 ->
// 172 TFLOP/s at the cfg-3 shapes): (i) staging registers declared as HIP's float4 were split into
// scalars and re-assembled with v_mov right after the load -- behind an s_waitcnt vmcnt(0) that drained
// the whole four-tile prefetch queue once per step; a native ext_vector_type(4) stays one register tuple
// (check the loop for vmcnt(0) after every change); (ii) the optional row gather's dependent index load
// costs the same drain, so it is a separate instantiation.  Row-contiguous operands: first (k pair) x
// (4 rows) micro-tiles written transposed with ds_write_b32 (2-way bank conflicts for any 16-byte-aligned
// row stride), now a straight [k][m] copy read back with ds_read_b64_tr_b16; (4 k) x (2 rows) micro-tiles
// with 8-byte global loads ran at 68 TFLOP/s (twice the load instructions).
#include <algorithm>

#include "common.h"
#include "gemm_f32.h"
#include "gemm_h16_dev.h"

namespace sctc {

static constexpr int S3_BM = 128, S3_BN = 128, S3_NT = 256, S3_BK = 16, S3_LD = S3_BK + 8;   // 48-byte LDS rows
static constexpr int S3_D = 4;                       // prefetch distance in K tiles (register sets)
#ifndef SCTC_S3_GR
#define SCTC_S3_GR 8
#endif
static constexpr int S3_GR = SCTC_S3_GR;             // tile rows per band of the block -> tile order
// Row-contiguous operands ([k][m] in memory: the weight gradient's deltas and activations, the delta
// propagation's weights) keep that orientation in LDS -- [k][m] with a k-row stride of 160 halves
// (320 B: the 4 k-rows x 32 B that a 16-lane group of ds_read_b64_tr_b16 touches, and the second group
// of the same 32-lane half 32 B further, cover the 64 banks once) -- and are turned into K-contiguous
// MFMA fragments by the hardware transpose read: the 16 lanes of a group supply the addresses of a
// [4 k][16 m] block, 4 consecutive m each (lane i: k = i / 4, m = 4 (i % 4)), and lane i receives
// column i's 4 k.  Staging is then the same straight copy as for K-contiguous operands (float4 = 4
// consecutive m at one k -> one ds_write_b64 per plane, conflict-free).  The transposing WRITE this
// replaces -- (k pair) x (4 rows) micro-tiles, 24 ds_write_b32 per step with 2-way bank conflicts --
// held the weight gradient at 122 TFLOP/s (3362 cycles per step) against 168 forward.
static constexpr int S3_RS = 160;
typedef __attribute__((address_space(3))) b16x4 lds_b16x4;
static constexpr int S3_OP = S3_BM * S3_LD;          // halves per operand plane (S3_BM == S3_BN)
static constexpr int S3_BUF = 6 * S3_OP;             // halves per buffer: A planes 0..2, B planes 0..2

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // staging registers: a native 128-bit tuple (HIP's float4
                                                            // was split into scalars and re-assembled with v_mov after
                                                            // the load, each time behind an s_waitcnt vmcnt(0))
typedef __bf16 b16x2 __attribute__((ext_vector_type(2)));

// exact three-term split of two floats; term t of both packed into one dword (element 0 low).
// 9 VALU per pair: v_cvt_pk_bf16_f32, shift + and back to fp32, v_pk_add_f32 -- twice, + the last convert
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t (&t)[3])
{
    f32x2 x = {a, b};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const b16x2 h = __builtin_convertvector(x, b16x2);
        t[k] = __builtin_bit_cast(uint32_t, h);
        if (k < 2) {
            const f32x2 f = {__uint_as_float(t[k] << 16), __uint_as_float(t[k] & 0xffff0000u)};
            x = x - f;
        }
    }
}

// four consecutive k of one row -> the three planes (one ds_write_b64 each)
__device__ __forceinline__ void put4(unsigned short* dst, float x0, float x1, float x2, float x3)
{
    uint32_t lo[3], hi[3];
    split3_pair(x0, x1, lo);
    split3_pair(x2, x3, hi);
#pragma unroll
    for (int t = 0; t < 3; ++t) *reinterpret_cast<u32x2*>(dst + t * S3_OP) = u32x2{lo[t], hi[t]};
}

// GATHER: a row-contiguous operand's k rows go through idx_a / idx_b (the recurrent weight gradient of
// a ragged minibatch pairs frame t with t+-1 through index lists).  An index fetched right before its
// use costs an s_waitcnt vmcnt(0) per re-load -- it drains the whole prefetch queue -- so (i) the common
// case is a separate instantiation without any index, (ii) the gather variant fetches the index of a
// staging register's NEXT tile when it issues the current one (tiles are loaded in increasing order).
template <bool AK, bool BKC, bool GATHER>
__global__ __launch_bounds__(S3_NT, 2) void gemm_s3_kernel(GemmArgs p)
{
    constexpr int TM = 2, TN = 2;
    using HT = H16<true>;
    extern __shared__ __attribute__((aligned(16))) unsigned short hsmem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int M = p.M, N = p.N, K = p.K;
    const int mt = (M + S3_BM - 1) / S3_BM, nt = (N + S3_BN - 1) / S3_BN;
    // tile order: an XCD walks consecutive entries of a list that runs through the output in bands of
    // S3_GR tile rows, column by column inside a band -- its ~64 concurrently resident blocks then cover
    // about 8 x 8 tiles (8 A panels + 8 B panels in its L2) instead of 4 full rows (4 + nt panels)
    const int swz = h16_swizzle(mt * nt);
    const int band = swz / (S3_GR * nt), inb = swz - band * (S3_GR * nt);
    const int rows = min(S3_GR, mt - band * S3_GR);
    const int tile_m = band * S3_GR + inb % rows, tile_n = inb / rows;
    const int m0 = tile_m * S3_BM, n0 = tile_n * S3_BN;
    const int ktiles = (K + S3_BK - 1) / S3_BK;
    const int per = (ktiles + p.splits - 1) / p.splits;
    const int kt_beg = blockIdx.y * per;
    const int kt_end = min(ktiles, kt_beg + per);

    f32x16 acc[TM][TN];
    static_for<TM * TN>([&](auto IJ) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[decltype(IJ)::value / TN][decltype(IJ)::value % TN][r] = 0.f;
    });

    const bool do_colsum = !AK && p.colsum_a != nullptr && tile_n == 0;
    float asum[4] = {0.f, 0.f, 0.f, 0.f};    // row-contiguous A: sums over k of this thread's 4 columns (m)
    // staging: 2 float4 per thread, operand and K tile
    //   K-contiguous  : k quad kq = tid & 3, rows (tid >> 2) + 64 q        (float4 = 4 k of one row)
    //   row-contiguous: m quad mq = tid & 31, k = (tid >> 5) + 8 q         (float4 = 4 m of one k)
    const int kq = tid & 3, mq = tid & 31, kr = tid >> 5;
    if (kt_beg < kt_end) {
        f32x4 sa[S3_D][2], sb[S3_D][2];
        const int Kc4 = (K - 1) & ~3, Kc1 = K - 1;
        const float* pa[2];
        const float* pb[2];
        if constexpr (AK) {
#pragma unroll
            for (int q = 0; q < 2; ++q) pa[q] = p.A + (int64_t)min(m0 + (tid >> 2) + 64 * q, M - 1) * p.lda;
        } else {
            pa[0] = p.A + min(m0 + 4 * mq, (M - 1) & ~3);
        }
        if constexpr (BKC) {
#pragma unroll
            for (int q = 0; q < 2; ++q) pb[q] = p.B + (int64_t)min(n0 + (tid >> 2) + 64 * q, N - 1) * p.ldb;
        } else {
            pb[0] = p.B + min(n0 + 4 * mq, (N - 1) & ~3);
        }
        // gather variant: ia[q] / ib[q] = row of the NEXT tile that staging piece q will load
        int ia[2] = {0, 0}, ib[2] = {0, 0};
        if constexpr (GATHER) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = min(kt_beg * S3_BK + kr + 8 * q, Kc1);
                ia[q] = (!AK && p.idx_a) ? p.idx_a[k] : k;
                ib[q] = (!BKC && p.idx_b) ? p.idx_b[k] : k;
            }
        }
        // unconditional loads from clamped addresses (tiles past the end re-read valid elements); every
        // staging piece q is loaded for consecutive tiles kt_beg, kt_beg + 1, ... in this order
        auto load_a = [&](f32x4& dst, int q, int kt) {
            const int k0 = kt * S3_BK;
            if constexpr (AK) {
                dst = *reinterpret_cast<const f32x4*>(pa[q] + min(k0 + 4 * kq, Kc4));
            } else if constexpr (GATHER) {
                dst = *reinterpret_cast<const f32x4*>(pa[0] + (uint32_t)ia[q] * (uint32_t)p.lda);
                const int kn = min(k0 + S3_BK + kr + 8 * q, Kc1);
                ia[q] = p.idx_a ? p.idx_a[kn] : kn;
            } else {
                dst = *reinterpret_cast<const f32x4*>(pa[0] + (uint32_t)min(k0 + kr + 8 * q, Kc1) * (uint32_t)p.lda);
            }
        };
        auto load_b = [&](f32x4& dst, int q, int kt) {
            const int k0 = kt * S3_BK;
            if constexpr (BKC) {
                dst = *reinterpret_cast<const f32x4*>(pb[q] + min(k0 + 4 * kq, Kc4));
            } else if constexpr (GATHER) {
                dst = *reinterpret_cast<const f32x4*>(pb[0] + (uint32_t)ib[q] * (uint32_t)p.ldb);
                const int kn = min(k0 + S3_BK + kr + 8 * q, Kc1);
                ib[q] = p.idx_b ? p.idx_b[kn] : kn;
            } else {
                dst = *reinterpret_cast<const f32x4*>(pb[0] + (uint32_t)min(k0 + kr + 8 * q, Kc1) * (uint32_t)p.ldb);
            }
        };
        // K tail: the A elements beyond K are zeroed (their B partners are finite re-reads)
        auto fix_tail = [&](f32x4 (&x)[2], int kt) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const bool z = AK ? (kt * S3_BK + 4 * kq >= K) : (kt * S3_BK + kr + 8 * q >= K);
                if (z) x[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        const int li = lane & 31, kg = lane >> 5;
        // fragment addresses (halves from the start of a buffer; plane t at + t * S3_OP, B planes after A's)
        //   K-contiguous  : one ds_read_b128, lane l holds row l & 31, 8 consecutive k at 8 * (l >> 5)
        //   row-contiguous: two ds_read_b64_tr_b16 (k .. k+3 and k+4 .. k+7 of the lane's k half)
        const int tr_off = (8 * kg + ((lane & 15) >> 2)) * S3_RS + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        const int aoff = AK ? (wm * 64 + li) * S3_LD + 8 * kg : tr_off + wm * 64;
        const int boff = 3 * S3_OP + (BKC ? (wn * 64 + li) * S3_LD + 8 * kg : tr_off + wn * 64);
        auto frag = [&](auto KC, const unsigned short* base, int off, int tile) -> b16x8 {
            if constexpr (decltype(KC)::value) {
                return *reinterpret_cast<const b16x8*>(base + off + tile * 32 * S3_LD);
            } else {
                const unsigned short* q = base + off + tile * 32;
                const b16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b16x4*)q);
                const b16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b16x4*)(q + 4 * S3_RS));
                const u32x2 l2 = __builtin_bit_cast(u32x2, lo4), h2 = __builtin_bit_cast(u32x2, hi4);
                const u32x4 v = {l2[0], l2[1], h2[0], h2[1]};
                return __builtin_bit_cast(b16x8, v);
            }
        };
        // LDS destinations of the staging registers, halves from the start of an operand's plane 0
        const int dst_a0 = AK ? (tid >> 2) * S3_LD + 4 * kq : kr * S3_RS + 4 * mq;
        const int dst_b0 = BKC ? (tid >> 2) * S3_LD + 4 * kq : kr * S3_RS + 4 * mq;
        constexpr int DA = AK ? 64 * S3_LD : 8 * S3_RS, DB = BKC ? 64 * S3_LD : 8 * S3_RS;
        uint32_t lo[3], hi[3];
        // One piece of an operand's re-staging (tile in register set x -> LDS planes at `out`), u = 0..7:
        // per float4 q [split x,y | split z,w | three ds_write_b64 | re-load with tile kt_next]
        auto sub_op = [&](auto ISA, auto U, f32x4 (&x)[2], unsigned short* out, bool live, int kt_next) {
            constexpr bool isA = decltype(ISA)::value;
            constexpr int u = decltype(U)::value;
            unsigned short* dst = out + (isA ? dst_a0 : 3 * S3_OP + dst_b0);
            constexpr int D = isA ? DA : DB;
            if constexpr (u < 8) {
                constexpr int q = u / 4, part = u % 4;
                if constexpr (part == 0) {
                    split3_pair(x[q].x, x[q].y, lo);
                    if constexpr (isA && !AK) {     // bias gradient: exact fp32 sums of the deltas, branch-free
                        const bool on = live && do_colsum;
                        asum[0] += on ? x[q].x : 0.f;
                        asum[1] += on ? x[q].y : 0.f;
                        asum[2] += on ? x[q].z : 0.f;
                        asum[3] += on ? x[q].w : 0.f;
                    }
                }
                if constexpr (part == 1) split3_pair(x[q].z, x[q].w, hi);
                if constexpr (part == 2) {
#pragma unroll
                    for (int t = 0; t < 3; ++t) *reinterpret_cast<u32x2*>(dst + q * D + t * S3_OP) = u32x2{lo[t], hi[t]};
                }
                if constexpr (part == 3) { if constexpr (isA) load_a(x[q], q, kt_next); else load_b(x[q], q, kt_next); }
            }
        };
        using TrueT = std::integral_constant<bool, true>;
        using FalseT = std::integral_constant<bool, false>;
        // One pipelined step (relative tile index j = kt - kt_beg, R = j % S3_D compile-time): the 24
        // MFMAs of tile j from LDS buffer j & 1; slots 0..11 re-stage the A operand of tile j + 1 (register
        // set (j + 1) % S3_D -> buffer (j + 1) & 1) and re-load the set with tile j + 1 + S3_D, slots
        // 12..23 the B operand.
        auto step = [&](auto RR, int kt) {
            constexpr int R = decltype(RR)::value, P = R & 1, Q = (R + 1) % S3_D;
            if ((kt + 2) * S3_BK > K && kt + 1 < kt_end) fix_tail(sa[Q], kt + 1);   // uniform, last tile only
            const unsigned short* base = hsmem + P * S3_BUF;
            unsigned short* out = hsmem + (P ^ 1) * S3_BUF;
            const bool live = kt + 1 < kt_end;
            b16x8 af[3][TM], bf[3][TN];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[t][i] = frag(std::integral_constant<bool, AK>{}, base, aoff + t * S3_OP, i);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[t][j] = frag(std::integral_constant<bool, BKC>{}, base, boff + t * S3_OP, j);
            }
            __builtin_amdgcn_sched_barrier(0);
            static_for<24>([&](auto SI) {
                constexpr int sl = decltype(SI)::value;
                constexpr int t = sl / 4, i = (sl % 4) / TN, j = sl % TN;
                // (A term, B term), smallest products first: x1y3, x3y1, x2y2, x1y2, x2y1, x1y1
                constexpr int ta = t == 0 ? 0 : t == 1 ? 2 : t == 2 ? 1 : t == 3 ? 0 : t == 4 ? 1 : 0;
                constexpr int tb = t == 0 ? 2 : t == 1 ? 0 : t == 2 ? 1 : t == 3 ? 1 : t == 4 ? 0 : 0;
                // operands swapped: the accumulator tile is the transpose of the output block (h16_epilogue)
                acc[i][j] = HT::mfma(bf[tb][j], af[ta][i], acc[i][j]);
                if constexpr (sl < 12) sub_op(TrueT{}, std::integral_constant<int, sl>{}, sa[Q], out, live, kt + 1 + S3_D);
                else sub_op(FalseT{}, std::integral_constant<int, sl - 12>{}, sb[Q], out, live, kt + 1 + S3_D);
                __builtin_amdgcn_sched_barrier(0);
            });
            __syncthreads();
        };

        // prologue: tiles 0 .. S3_D-1 into their register sets, tile 0 into LDS buffer 0 (its set is
        // re-loaded with tile S3_D)
        static_for<S3_D>([&](auto J) {
            constexpr int jj = decltype(J)::value;
#pragma unroll
            for (int q = 0; q < 2; ++q) { load_a(sa[jj][q], q, kt_beg + jj); load_b(sb[jj][q], q, kt_beg + jj); }
        });
        if ((kt_beg + 1) * S3_BK > K) fix_tail(sa[0], kt_beg);
        static_for<12>([&](auto U) { sub_op(TrueT{}, U, sa[0], hsmem, true, kt_beg + S3_D); });
        static_for<12>([&](auto U) { sub_op(FalseT{}, U, sb[0], hsmem, true, kt_beg + S3_D); });
        __syncthreads();
#ifdef SCTC_S3_STAMP
        uint64_t st_c0 = 0, st_w0 = 0;
        if (tid == 0) { st_c0 = __builtin_amdgcn_s_memtime(); st_w0 = __builtin_amdgcn_s_memrealtime(); }
#endif
        for (int kt = kt_beg; kt < kt_end; kt += S3_D) {
            step(std::integral_constant<int, 0>{}, kt);
            if (kt + 1 < kt_end) step(std::integral_constant<int, 1>{}, kt + 1);
            if (kt + 2 < kt_end) step(std::integral_constant<int, 2>{}, kt + 2);
            if (kt + 3 < kt_end) step(std::integral_constant<int, 3>{}, kt + 3);
        }
#ifdef SCTC_S3_STAMP
        // diagnostics build (tests/gpu_diag.py s3stamp): shader cycles and 100 MHz wall ticks of the main loop
        if (tid == 0 && blockIdx.x < 64 && p.splitk_ws && p.splits == 1) {
            const uint64_t c1 = __builtin_amdgcn_s_memtime(), w1 = __builtin_amdgcn_s_memrealtime();
            uint32_t* o = reinterpret_cast<uint32_t*>(p.splitk_ws) + 4 * blockIdx.x;
            o[0] = (uint32_t)(c1 - st_c0); o[1] = (uint32_t)(w1 - st_w0); o[2] = (uint32_t)(kt_end - kt_beg); o[3] = 1;
        }
#endif
    }
    if constexpr (!AK) {
        if (do_colsum) {       // block-uniform: the 8 threads that share an m quad (kr = 0..7) add up via LDS
            __syncthreads();
            float* red = reinterpret_cast<float*>(hsmem);          // [8][128]
#pragma unroll
            for (int c = 0; c < 4; ++c) red[kr * 128 + 4 * mq + c] = asum[c];
            __syncthreads();
            if (tid < 128) {
                float v = 0.f;
#pragma unroll
                for (int r = 0; r < 8; ++r) v += red[r * 128 + tid];
                const int m = m0 + tid;
                if (m < p.M) {
                    if (p.splits > 1)
                        p.splitk_ws[(int64_t)p.splits * p.M * p.N + (int64_t)blockIdx.y * p.M + m] = v;
                    else
                        p.colsum_a[m] = p.accumulate ? p.colsum_a[m] + v : v;
                }
            }
        }
    }
    h16_epilogue<TM, TN>(p, acc, m0, n0, wm, wn, lane);
}

// ------------------------------------------------------------------ host side

GemmKernelFn gemm_s3_kernel_for(const GemmPlan& p)
{
    static_assert(S3_BM == GEMM_S3_TILE && S3_BN == GEMM_S3_TILE && S3_BK == GEMM_S3_BK && S3_NT == 256 &&
                  sizeof(unsigned short) * 2 * S3_BUF == GEMM_S3_LDS, "gemm_plan.h, GEMM_S3_*: out of date");
    const bool g = p.gather;      // the K-contiguous pair has no row to gather
    if (p.ak) return p.bkc ? gemm_s3_kernel<true, true, false> : (g ? gemm_s3_kernel<true, false, true> : gemm_s3_kernel<true, false, false>);
    if (p.bkc) return g ? gemm_s3_kernel<false, true, true> : gemm_s3_kernel<false, true, false>;
    return g ? gemm_s3_kernel<false, false, true> : gemm_s3_kernel<false, false, false>;
}

}  // namespace sctc
