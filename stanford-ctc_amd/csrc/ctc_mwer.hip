// Minimum word error rate training over n-best lists (the contract is stated in include/sctc.h, the
// caller is ctc_torch.mwer_loss).  Utterance n of a time-major [T, N, C] tensor has up to K hypotheses; the loss is the
// expected error under the model's own posterior over them, and its gradient needs the CTC occupancies of all K label
// rows over the same frames.  A buffer [T][N * K][C] is a batch of sctc_ctc_loss_batch as it stands: frame t of
// hypothesis k of utterance n is row rowbase[t] + frame_off[n * K + k] with rowbase[t] = t * N * K and frame_off = n * K +
// k -- so the K * C elements of one (t, n) are contiguous.  Three kernels around that call, none with atomics or a wait
// for another workgroup:
//
//   ctc_mwer_probs_kernel    §4.13's prologue (ctc_tnc.hip restated: that file stays as it is): the probabilities of a
//                            (t, n) computed ONCE from the strided input and stored to the K_n[n] rows of its ranks.
//                            A row per lane for C <= 32, a row per wave beyond.  Padded frames and ranks >= K_n are
//                            neither read nor written.
//   ctc_mwer_coef_kernel     one wave per utterance, four per workgroup (nbest_mbr_kernel's shape): which ranks are
//                            real, the posterior over them, the expected error, the loss and d loss / d ll_k.  float64,
//                            sums in ascending k, no contraction.
//   ctc_mwer_combine_kernel  G[t * N + n][c] = sum over the real k, ascending, of coef_k * (p - g_k): the K gradient rows
//                            of a (t, n) folded into one.  Rows of ranks that are not real are never read (they hold
//                            probabilities, zeros or nothing): by select.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "xlane.h"

namespace sctc {
namespace {

constexpr int MWER_THREADS = 256;
constexpr int MWER_LANE_MAX_C = 32;     // widest row of the row-per-lane mapping (ctc_tnc.hip's cut)
constexpr int MWER_MAX_BLOCKS = 256 * 32;
constexpr int MWER_MAX_K = 256;         // NBEST_MAX_K

struct MwerArgs {
    const void* x;          // probs: the strided [T, N, C] input
    void* y;                // probs: [T * N * K][C]; combine: G [T * N][C]
    const void* p;          // combine: the probabilities [T * N * K][C]
    const void* g;          // combine: the CTC gradient rows, same layout
    const int32_t* T_n;
    const int32_t* K_n;
    const double* cost;     // coef: [N * K]
    const int32_t* skip;    // coef: [N * K]
    const double* errors;   // coef: [N * K]
    double* loss;           // coef: [N]
    double* coef;           // coef out / combine in: [N * K]
    double* post;           // coef: [N * K]
    double* expected;       // coef: [N]
    int32_t* real;          // coef out / combine in: [N * K]
    int32_t* inactive;      // coef out / combine in: [N]
    double scale;
    int64_t st, sn, sc;
    int64_t rows;           // T * N
    int32_t N, K, C, subtract_mean;
};

__device__ __forceinline__ float mwer_exp(float v) { return expf(v); }
__device__ __forceinline__ double mwer_exp(double v) { return exp(v); }

// NA as in ctc_tnc_probs_kernel: registers per lane of the row-per-wave mapping (rows of up to 64 * NA columns); 0: any
// width, the row is read three times; -1: the row-per-lane mapping.  The arithmetic of a row is that kernel's, operation
// for operation, so a row here is bit-equal to the row ctc_loss forms from the same input.
template <typename R, int MODE, int NA>
__global__ __launch_bounds__(MWER_THREADS) void ctc_mwer_probs_kernel(MwerArgs p)
{
    const R* x = (const R*)p.x;
    R* y = (R*)p.y;
    const int C = p.C, K = p.K;
    const unsigned N = (unsigned)p.N;
    const int64_t sc = p.sc;
    const int64_t kc = (int64_t)K * C;      // from (t, n) to the next: r = t * N + n owns rows r * K .. r * K + K - 1
    if constexpr (NA < 0) {
        const int64_t step = (int64_t)gridDim.x * MWER_THREADS;
        for (int64_t r = (int64_t)blockIdx.x * MWER_THREADS + threadIdx.x; r < p.rows; r += step) {
            const unsigned t = (unsigned)r / N, n = (unsigned)r - t * N;
            if ((int)t >= p.T_n[n]) continue;
            const int kn = min(p.K_n[n], K);
            if (kn <= 0) continue;
            const R* xr = x + (int64_t)t * p.st + (int64_t)n * p.sn;
            R* yr = y + r * kc;
            R v[MWER_LANE_MAX_C];
            R m = -INFINITY;
#pragma unroll
            for (int k = 0; k < MWER_LANE_MAX_C; ++k) {
                v[k] = k < C ? xr[k * sc] : (R)-INFINITY;
                m = v[k] > m ? v[k] : m;
            }
            if constexpr (MODE == SCTC_TNC_LOGITS) {
                R s = 0;
#pragma unroll
                for (int k = 0; k < MWER_LANE_MAX_C; ++k) {
                    v[k] = k < C ? mwer_exp(v[k] - m) : (R)0;
                    s += v[k];
                }
                const R inv = (R)1 / s;
#pragma unroll
                for (int k = 0; k < MWER_LANE_MAX_C; ++k) v[k] = v[k] * inv;
            } else {
#pragma unroll
                for (int k = 0; k < MWER_LANE_MAX_C; ++k) v[k] = k < C ? mwer_exp(v[k]) : (R)0;
            }
            for (int h = 0; h < kn; ++h) {
                R* yh = yr + (int64_t)h * C;
#pragma unroll
                for (int k = 0; k < MWER_LANE_MAX_C; ++k)
                    if (k < C) yh[k] = v[k];
            }
        }
    } else {
        const int lane = threadIdx.x & 63;
        const int64_t step = (int64_t)gridDim.x * (MWER_THREADS / 64);
        for (int64_t r = (int64_t)blockIdx.x * (MWER_THREADS / 64) + (threadIdx.x >> 6); r < p.rows; r += step) {
            const unsigned t = (unsigned)r / N, n = (unsigned)r - t * N;
            if ((int)t >= __builtin_amdgcn_readfirstlane(p.T_n[n])) continue;    // the whole wave: r is wave-uniform
            const int kn = min(__builtin_amdgcn_readfirstlane(p.K_n[n]), K);
            if (kn <= 0) continue;
            const R* xr = x + (int64_t)t * p.st + (int64_t)n * p.sn;
            R* yr = y + r * kc;
            if constexpr (MODE == SCTC_TNC_LOG_PROBS) {
                for (int k = lane; k < C; k += 64) {
                    const R v = mwer_exp(xr[k * sc]);
                    for (int h = 0; h < kn; ++h) yr[(int64_t)h * C + k] = v;
                }
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
                    v[q] = k < C ? mwer_exp(v[q] - m) : (R)0;
                    s += v[q];
                }
                s = wave_sum(s);
                const R inv = (R)1 / s;
#pragma unroll
                for (int q = 0; q < NA; ++q) v[q] = v[q] * inv;
                for (int h = 0; h < kn; ++h) {
                    R* yh = yr + (int64_t)h * C;
#pragma unroll
                    for (int q = 0; q < NA; ++q) {
                        const int k = lane + 64 * q;
                        if (k < C) yh[k] = v[q];
                    }
                }
            } else {
                R m = -INFINITY;
                for (int k = lane; k < C; k += 64) {
                    const R v = xr[k * sc];
                    m = v > m ? v : m;
                }
                m = wave_max(m);
                R s = 0;
                for (int k = lane; k < C; k += 64) s += mwer_exp(xr[k * sc] - m);
                s = wave_sum(s);
                const R inv = (R)1 / s;
                for (int k = lane; k < C; k += 64) {
                    const R v = mwer_exp(xr[k * sc] - m) * inv;
                    for (int h = 0; h < kn; ++h) yr[(int64_t)h * C + k] = v;
                }
            }
        }
    }
}

__device__ __forceinline__ void mwer_wave_sync_lds()
{
    // every lane reads what every lane of this wave wrote
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(256) void ctc_mwer_coef_kernel(MwerArgs p)
{
#pragma clang fp contract(off)
    __shared__ double s_w[4][MWER_MAX_K], s_e[4][MWER_MAX_K];
    __shared__ int s_real[4][MWER_MAX_K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 4 + wave;
    if (n >= p.N) return;       // whole waves leave; there is no workgroup barrier below
    const int K = p.K, kn = min(p.K_n[n], K);
    double* w = s_w[wave];      // the weight of a rank, +0.0 where it is not real
    double* e = s_e[wave];      // its error, +0.0 where it is not real
    int* real = s_real[wave];   // a weight may underflow to 0: the flag is kept apart
    double mx = -INFINITY;
    int n_real = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane, kk = min(k, K - 1);
        const double cost = p.cost[n * K + kk], err = p.errors[n * K + kk];
        const bool r = k < kn && isfinite(err) && p.skip[n * K + kk] == 0 && isfinite(cost);
        const double ll = -cost;
        mx = r && ll > mx ? ll : mx;
        n_real += __popcll(__ballot(r));
        if (k < K) {
            real[k] = r;
            e[k] = r ? err : 0.0;
        }
    }
    mx = wave_max(mx);
    const bool active = p.T_n[n] >= 2 && n_real > 0;
    for (int k = lane; k < K; k += 64) {
        const bool r = real[k] != 0;        // this lane's own store
        const double ll = -p.cost[n * K + k];
        const double v = exp(p.scale * (ll - mx));
        w[k] = r ? (ll == mx ? 1.0 : v) : 0.0;      // exactly 1.0 at the maximum, whatever exp(0) gives (§4.15's rule)
    }
    mwer_wave_sync_lds();
    double Z = 0.0, wsum = 0.0;
    for (int k = 0; k < K; ++k) {           // ascending; a rank that is not real adds +0.0
        Z += w[k];
        wsum += e[k];
    }
    double R = 0.0;
    for (int k = 0; k < K; ++k) R += w[k] / Z * e[k];       // P_k * W_k; +0.0 from a rank that is not real
    if (!active) R = 0.0;       // without a real rank Z is 0
    const double wbar = wsum / (double)n_real;
    for (int k = lane; k < K; k += 64) {
        const bool r = active && real[k] != 0;
        const double P = w[k] / Z;
        p.post[n * K + k] = r ? P : 0.0;
        p.coef[n * K + k] = r ? p.scale * P * (e[k] - R) : 0.0;
        p.real[n * K + k] = r ? 1 : 0;
    }
    if (lane == 0) {
        p.loss[n] = active ? (p.subtract_mean ? R - wbar : R) : 0.0;
        p.expected[n] = R;
        p.inactive[n] = active ? 0 : 1;
    }
}

// A wave takes 64 / G consecutive (t, n), G = the power of two >= C (64 for wider rows): lane -> ((t, n), column) by shift
// and mask.  The K * C elements of a (t, n) are contiguous, so the wave reads whole lines at every C.  p is the same in
// every rank's row of a (t, n): it is read once, from the first real rank's row.
template <typename R>
__global__ __launch_bounds__(MWER_THREADS) void ctc_mwer_combine_kernel(MwerArgs p, int shift)
{
#pragma clang fp contract(off)
    const R* pr = (const R*)p.p;
    const R* g = (const R*)p.g;
    R* out = (R*)p.y;
    const int C = p.C, K = p.K, G = 1 << shift;
    const unsigned N = (unsigned)p.N;
    const int lane = threadIdx.x & 63;
    const int sub = lane >> shift, c0 = lane & (G - 1), rpw = 64 >> shift;
    const int64_t step = (int64_t)gridDim.x * (MWER_THREADS / 64) * rpw;
    for (int64_t r = ((int64_t)blockIdx.x * (MWER_THREADS / 64) + (threadIdx.x >> 6)) * rpw + sub; r < p.rows; r += step) {
        const unsigned t = (unsigned)r / N, n = (unsigned)r - t * N;
        if ((int)t >= p.T_n[n] || p.inactive[n] != 0) continue;
        const int64_t base = r * K * C;
        const double* coef = p.coef + (int64_t)n * K;
        const int32_t* real = p.real + (int64_t)n * K;
        int first = 0;
        while (first < K - 1 && !real[first]) ++first;     // an active utterance has a real rank
        for (int c = c0; c < C; c += G) {
            const double pv = (double)pr[base + (int64_t)first * C + c];
            double acc = 0.0;
            for (int k = 0; k < K; ++k)
                if (real[k]) acc += coef[k] * (pv - (double)g[base + (int64_t)k * C + c]);
            out[r * C + c] = (R)acc;
        }
    }
}

int mwer_check(const sctc_mwer_config* cfg, const char* what)
{
    SCTC_CHECK_ARG(cfg, "%s: null config", what);
    SCTC_CHECK_ARG(cfg->T >= 0 && cfg->N >= 0, "%s: T = %d, N = %d", what, cfg->T, cfg->N);
    SCTC_CHECK_ARG(cfg->K >= 1 && cfg->K <= MWER_MAX_K, "%s: K = %d hypotheses outside 1..%d", what, cfg->K, MWER_MAX_K);
    SCTC_CHECK_ARG(cfg->C >= 1, "%s: alphabet of %d symbols", what, cfg->C);
    SCTC_CHECK_ARG(cfg->dtype == SCTC_F32 || cfg->dtype == SCTC_F64, "%s: dtype %d is neither SCTC_F32 nor SCTC_F64", what,
                   cfg->dtype);
    SCTC_CHECK_ARG(cfg->mode == SCTC_TNC_LOG_PROBS || cfg->mode == SCTC_TNC_LOGITS, "%s: mode %d is neither SCTC_TNC_LOG_PROBS nor "
                   "SCTC_TNC_LOGITS", what, cfg->mode);
    SCTC_CHECK_ARG((int64_t)cfg->T * cfg->N * cfg->K <= INT32_MAX, "%s: T * N * K = %lld rows do not fit the int32 row index", what,
                   (long long)cfg->T * cfg->N * cfg->K);
    SCTC_CHECK_ARG(std::isfinite(cfg->scale) && cfg->scale >= 0.0, "%s: scale %g is not finite or is negative", what, cfg->scale);
    SCTC_CHECK_ARG(cfg->subtract_mean == 0 || cfg->subtract_mean == 1, "%s: subtract_mean %d is neither 0 nor 1", what,
                   cfg->subtract_mean);
    return SCTC_OK;
}

MwerArgs mwer_args(const sctc_mwer_config* cfg, const int32_t* T_n, const int32_t* K_n)
{
    MwerArgs a{};
    a.T_n = T_n;
    a.K_n = K_n;
    a.scale = cfg->scale;
    a.st = cfg->stride_t;
    a.sn = cfg->stride_n;
    a.sc = cfg->stride_c;
    a.rows = (int64_t)cfg->T * cfg->N;
    a.N = cfg->N;
    a.K = cfg->K;
    a.C = cfg->C;
    a.subtract_mean = cfg->subtract_mean;
    return a;
}

template <typename R, int MODE>
void launch_probs(const MwerArgs& a, hipStream_t s)
{
    if (a.C <= MWER_LANE_MAX_C) {
        const unsigned grid = (unsigned)std::min<int64_t>((a.rows + MWER_THREADS - 1) / MWER_THREADS, MWER_MAX_BLOCKS);
        hipLaunchKernelGGL((ctc_mwer_probs_kernel<R, MODE, -1>), dim3(grid), dim3(MWER_THREADS), 0, s, a);
        return;
    }
    const unsigned grid = (unsigned)std::min<int64_t>((a.rows + 3) / 4, MWER_MAX_BLOCKS);
    if (a.C <= 64) hipLaunchKernelGGL((ctc_mwer_probs_kernel<R, MODE, 1>), dim3(grid), dim3(MWER_THREADS), 0, s, a);
    else if (a.C <= 128) hipLaunchKernelGGL((ctc_mwer_probs_kernel<R, MODE, 2>), dim3(grid), dim3(MWER_THREADS), 0, s, a);
    else if (a.C <= 256) hipLaunchKernelGGL((ctc_mwer_probs_kernel<R, MODE, 4>), dim3(grid), dim3(MWER_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ctc_mwer_probs_kernel<R, MODE, 0>), dim3(grid), dim3(MWER_THREADS), 0, s, a);
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_ctc_mwer_probs(const sctc_mwer_config* cfg, const void* input_dev, const int32_t* T_n_dev, const int32_t* K_n_dev,
                        void* probs_dev, void* stream)
{
    SCTC_TRY(mwer_check(cfg, "mwer_probs"));
    if (cfg->T == 0 || cfg->N == 0) return SCTC_OK;
    SCTC_CHECK_ARG(input_dev && T_n_dev && K_n_dev && probs_dev, "mwer_probs: null pointer");
    MwerArgs a = mwer_args(cfg, T_n_dev, K_n_dev);
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

int sctc_ctc_mwer_coef(const sctc_mwer_config* cfg, const double* cost_dev, const int32_t* skip_dev, const double* errors_dev,
                       const int32_t* T_n_dev, const int32_t* K_n_dev, double* loss_dev, double* coef_dev,
                       double* posterior_dev, double* expected_dev, int32_t* real_dev, int32_t* inactive_dev, void* stream)
{
    SCTC_TRY(mwer_check(cfg, "mwer_coef"));
    if (cfg->N == 0) return SCTC_OK;
    SCTC_CHECK_ARG(cost_dev && skip_dev && errors_dev && T_n_dev && K_n_dev && loss_dev && coef_dev && posterior_dev &&
                   expected_dev && real_dev && inactive_dev, "mwer_coef: null pointer");
    MwerArgs a = mwer_args(cfg, T_n_dev, K_n_dev);
    a.cost = cost_dev;
    a.skip = skip_dev;
    a.errors = errors_dev;
    a.loss = loss_dev;
    a.coef = coef_dev;
    a.post = posterior_dev;
    a.expected = expected_dev;
    a.real = real_dev;
    a.inactive = inactive_dev;
    hipLaunchKernelGGL(ctc_mwer_coef_kernel, dim3((unsigned)((cfg->N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

int sctc_ctc_mwer_combine(const sctc_mwer_config* cfg, const void* probs_dev, const void* grad_dev, const double* coef_dev,
                          const int32_t* real_dev, const int32_t* T_n_dev, const int32_t* inactive_dev, void* out_dev,
                          void* stream)
{
    SCTC_TRY(mwer_check(cfg, "mwer_combine"));
    if (cfg->T == 0 || cfg->N == 0) return SCTC_OK;
    SCTC_CHECK_ARG(probs_dev && grad_dev && coef_dev && real_dev && T_n_dev && inactive_dev && out_dev,
                   "mwer_combine: null pointer");
    MwerArgs a = mwer_args(cfg, T_n_dev, nullptr);
    a.p = probs_dev;
    a.g = grad_dev;
    a.coef = const_cast<double*>(coef_dev);
    a.real = const_cast<int32_t*>(real_dev);
    a.inactive = const_cast<int32_t*>(inactive_dev);
    a.y = out_dev;
    int shift = 0;
    while (shift < 6 && (1 << shift) < cfg->C) ++shift;
    const int64_t rows_per_block = (int64_t)(MWER_THREADS / 64) * (64 >> shift);
    const unsigned grid = (unsigned)std::min<int64_t>((a.rows + rows_per_block - 1) / rows_per_block, MWER_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    if (cfg->dtype == SCTC_F64) hipLaunchKernelGGL(ctc_mwer_combine_kernel<double>, dim3(grid), dim3(MWER_THREADS), 0, s, a, shift);
    else hipLaunchKernelGGL(ctc_mwer_combine_kernel<float>, dim3(grid), dim3(MWER_THREADS), 0, s, a, shift);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
