// What surrounds sctc_ctc_loss_batch when the batch is a time-major [T, N, C] tensor, the layout of
// torch.nn.functional.ctc_loss (the contract is stated in include/sctc.h, the caller is ctc_torch.py).
// A contiguous [T * N][C] buffer is already a batch of the CTC kernels: frame t of utterance n is row
// rowbase[t] + frame_off[n] with rowbase[t] = t * N and frame_off[n] = n.  Three kernels, none with atomics or a wait for
// another workgroup:
//
//   ctc_tnc_probs_kernel   the prologue: probabilities [T * N][C] from an input of any element strides; exp(x) of
//                          log-probabilities or the softmax of unnormalised activations (row max, exp, scale by 1 / sum:
//                          softmax_rows_kernel of ctc_kernels.hip, here in float64 too).  Rows are mapped to lanes as in
//                          ctc_bestpath.hip: a row per lane for C <= 32 (the row sits in registers, no cross-lane traffic),
//                          a row per wave beyond (lane k takes columns k, k + 64, ...).  The cut: a wave instruction of
//                          the lane mapping touches 64 rows C elements apart, so every 128-byte line it opens is used up
//                          over the next 128 / (C * sizeof) .. C iterations by the same wave -- up to 32 float32 columns
//                          that is at most one line per lane in flight (64 lines, 8 KiB of the CU's 32 KiB L1); beyond,
//                          the row per wave reads and writes whole lines with at least half of its lanes.
//   ctc_tnc_empty_kernel   utterances with an empty target, one wave each: -sum_t log p[t, n, blank] and the rows
//                          p - onehot(blank).  With a symbol per utterance in place of the blank it also takes the other
//                          utterance whose one alignment emits one symbol in every frame: one label in one frame, where
//                          the reference (and the CTC kernels with it) answers -log(p_blank + p_label).
//   ctc_tnc_grad_kernel    the backward pass: scale[n] * g[t, n, c] into a strided output, exactly 0 for padded frames and
//                          unusable utterances -- by select, the rows it zeroes are not read.
//
// Rows of padded frames (t >= T_n[n]) are skipped by the first two kernels: neither read nor written.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "xlane.h"

namespace sctc {
namespace {

constexpr int TNC_THREADS = 256;
constexpr int TNC_LANE_MAX_C = 32;      // widest row of the row-per-lane mapping
constexpr int TNC_MAX_BLOCKS = 256 * 32;

struct TncArgs {
    const void* x;          // strided [T, N, C] (probs: input, grad: unused)
    void* y;                // contiguous [T * N][C] (probs: output) or strided (grad: output)
    const void* g;          // grad / empty: contiguous [T * N][C]
    const int32_t* T_n;
    const int32_t* idx;     // empty: the utterances
    const int32_t* sym;     // empty: the symbol each of them emits in every frame (null: the blank)
    const double* cost;
    const int32_t* skip;
    const double* scale;
    double* cost_out;
    int32_t* skip_out;
    int64_t st, sn, sc;
    int64_t rows;           // T * N <= INT32_MAX
    int32_t N, C, blank;
};

__device__ __forceinline__ float tnc_exp(float v) { return expf(v); }
__device__ __forceinline__ double tnc_exp(double v) { return exp(v); }

// NA: registers per lane of the row-per-wave mapping (rows of up to 64 * NA columns); 0: any width, the row is read
// three times (softmax_rows_generic_kernel); -1: the row-per-lane mapping
template <typename R, int MODE, int NA>
__global__ __launch_bounds__(TNC_THREADS) void ctc_tnc_probs_kernel(TncArgs p)
{
    const R* x = (const R*)p.x;
    R* y = (R*)p.y;
    const int C = p.C;
    const unsigned N = (unsigned)p.N;
    const int64_t sc = p.sc;
    if constexpr (NA < 0) {
        const int64_t step = (int64_t)gridDim.x * TNC_THREADS;
        for (int64_t r = (int64_t)blockIdx.x * TNC_THREADS + threadIdx.x; r < p.rows; r += step) {
            const unsigned t = (unsigned)r / N, n = (unsigned)r - t * N;
            if ((int)t >= p.T_n[n]) continue;
            const R* xr = x + (int64_t)t * p.st + (int64_t)n * p.sn;
            R* yr = y + r * C;
            R v[TNC_LANE_MAX_C];
            R m = -INFINITY;
#pragma unroll
            for (int k = 0; k < TNC_LANE_MAX_C; ++k) {
                v[k] = k < C ? xr[k * sc] : (R)-INFINITY;
                m = v[k] > m ? v[k] : m;
            }
            if constexpr (MODE == SCTC_TNC_LOGITS) {
                R s = 0;
#pragma unroll
                for (int k = 0; k < TNC_LANE_MAX_C; ++k) {
                    v[k] = k < C ? tnc_exp(v[k] - m) : (R)0;
                    s += v[k];
                }
                const R inv = (R)1 / s;
#pragma unroll
                for (int k = 0; k < TNC_LANE_MAX_C; ++k)
                    if (k < C) yr[k] = v[k] * inv;
            } else {
#pragma unroll
                for (int k = 0; k < TNC_LANE_MAX_C; ++k)
                    if (k < C) yr[k] = tnc_exp(v[k]);
            }
        }
    } else {
        const int lane = threadIdx.x & 63;
        const int64_t step = (int64_t)gridDim.x * (TNC_THREADS / 64);
        for (int64_t r = (int64_t)blockIdx.x * (TNC_THREADS / 64) + (threadIdx.x >> 6); r < p.rows; r += step) {
            const unsigned t = (unsigned)r / N, n = (unsigned)r - t * N;
            if ((int)t >= __builtin_amdgcn_readfirstlane(p.T_n[n])) continue;    // the whole wave: r is wave-uniform
            const R* xr = x + (int64_t)t * p.st + (int64_t)n * p.sn;
            R* yr = y + r * C;
            if constexpr (MODE == SCTC_TNC_LOG_PROBS) {
                for (int k = lane; k < C; k += 64) yr[k] = tnc_exp(xr[k * sc]);
            } else if constexpr (NA > 0) {
                R v[NA];
                R m = -INFINITY;
#pragma unroll
                for (int q = 0; q < NA; ++q) {
                    const int k = lane + 64 * q;
                    v[q] = k < C ? xr[k * sc] : (R)-INFINITY;
                    m = v[q] > m ? v[q] : m;
                }
                m = wave_max(m);
                R s = 0;
#pragma unroll
                for (int q = 0; q < NA; ++q) {
                    const int k = lane + 64 * q;
                    v[q] = k < C ? tnc_exp(v[q] - m) : (R)0;
                    s += v[q];
                }
                s = wave_sum(s);
                const R inv = (R)1 / s;
#pragma unroll
                for (int q = 0; q < NA; ++q) {
                    const int k = lane + 64 * q;
                    if (k < C) yr[k] = v[q] * inv;
                }
            } else {
                R m = -INFINITY;
                for (int k = lane; k < C; k += 64) {
                    const R v = xr[k * sc];
                    m = v > m ? v : m;
                }
                m = wave_max(m);
                R s = 0;
                for (int k = lane; k < C; k += 64) s += tnc_exp(xr[k * sc] - m);
                s = wave_sum(s);
                const R inv = (R)1 / s;
                for (int k = lane; k < C; k += 64) yr[k] = tnc_exp(xr[k * sc] - m) * inv;
            }
        }
    }
}

template <typename R>
__global__ __launch_bounds__(64) void ctc_tnc_empty_kernel(TncArgs p)
{
    const int lane = threadIdx.x;
    const int n = p.idx[blockIdx.x];
    const int T = __builtin_amdgcn_readfirstlane(p.T_n[n]);
    const int C = p.C, sym = p.sym ? p.sym[blockIdx.x] : p.blank;
    const R* pr = (const R*)p.g;
    R* gr = (R*)p.y;
    const int64_t ldn = (int64_t)p.N * C;       // from frame t to frame t + 1 of one utterance
    const int64_t base = (int64_t)n * C;
    double acc = 0.0;
    bool zero = false;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        double lv = 0.0;
        if (t < T) {
            const double pb = (double)pr[base + t * ldn + sym];
            zero = zero || pb == 0.0;
            lv = log(pb);
        }
        const int cnt = min(64, T - t0);
        for (int i = 0; i < cnt; ++i) acc += __shfl(lv, i, 64);     // ascending t, whatever the lane count
    }
    const int64_t elems = (int64_t)T * C;
    for (int64_t i = lane; i < elems; i += 64) {
        const int64_t t = i / C;
        const int k = (int)(i - t * C);
        const int64_t e = base + t * ldn + k;
        gr[e] = pr[e] - (k == sym ? (R)1 : (R)0);
    }
    const bool any_zero = __ballot(zero) != 0ull;
    if (lane == 0) {
        p.cost_out[n] = any_zero ? (double)INFINITY : -acc;
        p.skip_out[n] = any_zero ? 1 : 0;
    }
}

// A wave takes 64 / G consecutive rows, G = the power of two >= C (64 for wider rows): lane -> (row, column) by shift
// and mask, rows of the contiguous gradient buffer read in whole lines at every C
template <typename R>
__global__ __launch_bounds__(TNC_THREADS) void ctc_tnc_grad_kernel(TncArgs p, int shift)
{
    const R* g = (const R*)p.g;
    R* out = (R*)p.y;
    const int C = p.C, G = 1 << shift;
    const unsigned N = (unsigned)p.N;
    const int lane = threadIdx.x & 63;
    const int sub = lane >> shift, c0 = lane & (G - 1), rpw = 64 >> shift;
    const int64_t step = (int64_t)gridDim.x * (TNC_THREADS / 64) * rpw;
    for (int64_t r = ((int64_t)blockIdx.x * (TNC_THREADS / 64) + (threadIdx.x >> 6)) * rpw + sub; r < p.rows; r += step) {
        const unsigned t = (unsigned)r / N, n = (unsigned)r - t * N;
        const double cost = p.cost[n];
        const bool live = (int)t < p.T_n[n] && p.skip[n] == 0 && isfinite(cost);
        const double scale = p.scale[n];
        R* orow = out + (int64_t)t * p.st + (int64_t)n * p.sn;
        for (int c = c0; c < C; c += G) {
            R v = (R)0;
            if (live) v = (R)(scale * (double)g[r * C + c]);
            orow[c * p.sc] = v;
        }
    }
}

int tnc_check(const sctc_tnc_config* cfg, const char* what)
{
    SCTC_CHECK_ARG(cfg, "%s: null config", what);
    SCTC_CHECK_ARG(cfg->T >= 0 && cfg->N >= 0, "%s: T = %d, N = %d", what, cfg->T, cfg->N);
    SCTC_CHECK_ARG(cfg->C >= 1, "%s: alphabet of %d symbols", what, cfg->C);
    SCTC_CHECK_ARG(cfg->blank >= 0 && cfg->blank < cfg->C, "%s: blank id %d outside the alphabet [0,%d)", what, cfg->blank, cfg->C);
    SCTC_CHECK_ARG(cfg->dtype == SCTC_F32 || cfg->dtype == SCTC_F64, "%s: dtype %d is neither SCTC_F32 nor SCTC_F64", what,
                   cfg->dtype);
    SCTC_CHECK_ARG(cfg->mode == SCTC_TNC_LOG_PROBS || cfg->mode == SCTC_TNC_LOGITS, "%s: mode %d is neither SCTC_TNC_LOG_PROBS nor "
                   "SCTC_TNC_LOGITS", what, cfg->mode);
    SCTC_CHECK_ARG((int64_t)cfg->T * cfg->N <= INT32_MAX, "%s: T * N = %lld rows do not fit the int32 row index", what,
                   (long long)cfg->T * cfg->N);
    return SCTC_OK;
}

TncArgs tnc_args(const sctc_tnc_config* cfg, const int32_t* T_n)
{
    TncArgs a{};
    a.T_n = T_n;
    a.st = cfg->stride_t;
    a.sn = cfg->stride_n;
    a.sc = cfg->stride_c;
    a.rows = (int64_t)cfg->T * cfg->N;
    a.N = cfg->N;
    a.C = cfg->C;
    a.blank = cfg->blank;
    return a;
}

template <typename R, int MODE>
void launch_probs(const TncArgs& a, hipStream_t s)
{
    if (a.C <= TNC_LANE_MAX_C) {
        const unsigned grid = (unsigned)std::min<int64_t>((a.rows + TNC_THREADS - 1) / TNC_THREADS, TNC_MAX_BLOCKS);
        hipLaunchKernelGGL((ctc_tnc_probs_kernel<R, MODE, -1>), dim3(grid), dim3(TNC_THREADS), 0, s, a);
        return;
    }
    const unsigned grid = (unsigned)std::min<int64_t>((a.rows + 3) / 4, TNC_MAX_BLOCKS);
    if (a.C <= 64) hipLaunchKernelGGL((ctc_tnc_probs_kernel<R, MODE, 1>), dim3(grid), dim3(TNC_THREADS), 0, s, a);
    else if (a.C <= 128) hipLaunchKernelGGL((ctc_tnc_probs_kernel<R, MODE, 2>), dim3(grid), dim3(TNC_THREADS), 0, s, a);
    else if (a.C <= 256) hipLaunchKernelGGL((ctc_tnc_probs_kernel<R, MODE, 4>), dim3(grid), dim3(TNC_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ctc_tnc_probs_kernel<R, MODE, 0>), dim3(grid), dim3(TNC_THREADS), 0, s, a);
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_ctc_tnc_probs(const sctc_tnc_config* cfg, const void* input_dev, const int32_t* T_n_dev, void* probs_dev,
                       void* stream)
{
    SCTC_TRY(tnc_check(cfg, "tnc_probs"));
    if (cfg->T == 0 || cfg->N == 0) return SCTC_OK;
    SCTC_CHECK_ARG(input_dev && T_n_dev && probs_dev, "tnc_probs: null pointer");
    TncArgs a = tnc_args(cfg, T_n_dev);
    a.x = input_dev;
    a.y = probs_dev;
    hipStream_t s = (hipStream_t)stream;
    const bool logits = cfg->mode == SCTC_TNC_LOGITS;
    if (cfg->dtype == SCTC_F64) {
        if (logits) launch_probs<double, SCTC_TNC_LOGITS>(a, s);
        else launch_probs<double, SCTC_TNC_LOG_PROBS>(a, s);
    } else {
        if (logits) launch_probs<float, SCTC_TNC_LOGITS>(a, s);
        else launch_probs<float, SCTC_TNC_LOG_PROBS>(a, s);
    }
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

int sctc_ctc_tnc_empty(const sctc_tnc_config* cfg, const void* probs_dev, const int32_t* T_n_dev, const int32_t* idx_dev,
                       const int32_t* sym_dev, int32_t n_idx, void* grad_dev, double* cost_dev, int32_t* skip_dev, void* stream)
{
    SCTC_TRY(tnc_check(cfg, "tnc_empty"));
    SCTC_CHECK_ARG(n_idx >= 0 && n_idx <= cfg->N, "tnc_empty: %d utterances listed, outside 0..%d", n_idx, cfg->N);
    if (cfg->T == 0 || cfg->N == 0 || n_idx == 0) return SCTC_OK;
    SCTC_CHECK_ARG(probs_dev && T_n_dev && idx_dev && grad_dev && cost_dev && skip_dev, "tnc_empty: null pointer");
    TncArgs a = tnc_args(cfg, T_n_dev);
    a.g = probs_dev;
    a.y = grad_dev;
    a.idx = idx_dev;
    a.sym = sym_dev;
    a.cost_out = cost_dev;
    a.skip_out = skip_dev;
    hipStream_t s = (hipStream_t)stream;
    if (cfg->dtype == SCTC_F64) hipLaunchKernelGGL(ctc_tnc_empty_kernel<double>, dim3((unsigned)n_idx), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(ctc_tnc_empty_kernel<float>, dim3((unsigned)n_idx), dim3(64), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

int sctc_ctc_tnc_grad(const sctc_tnc_config* cfg, const void* grad_dev, const int32_t* T_n_dev, const double* cost_dev,
                      const int32_t* skip_dev, const double* scale_dev, void* out_dev, void* stream)
{
    SCTC_TRY(tnc_check(cfg, "tnc_grad"));
    if (cfg->T == 0 || cfg->N == 0) return SCTC_OK;
    SCTC_CHECK_ARG(grad_dev && T_n_dev && cost_dev && skip_dev && scale_dev && out_dev, "tnc_grad: null pointer");
    TncArgs a = tnc_args(cfg, T_n_dev);
    a.g = grad_dev;
    a.y = out_dev;
    a.cost = cost_dev;
    a.skip = skip_dev;
    a.scale = scale_dev;
    int shift = 0;
    while (shift < 6 && (1 << shift) < cfg->C) ++shift;
    const int64_t rows_per_block = (int64_t)(TNC_THREADS / 64) * (64 >> shift);
    const unsigned grid = (unsigned)std::min<int64_t>((a.rows + rows_per_block - 1) / rows_per_block, TNC_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    if (cfg->dtype == SCTC_F64) hipLaunchKernelGGL(ctc_tnc_grad_kernel<double>, dim3(grid), dim3(TNC_THREADS), 0, s, a, shift);
    else hipLaunchKernelGGL(ctc_tnc_grad_kernel<float>, dim3(grid), dim3(TNC_THREADS), 0, s, a, shift);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
