// Minimum word error rate training inside the BRNN engine's step (the contract is stated in
// include/sctc.h, the caller is run_mwer of brnn_engine.hip).  The engine's probabilities lie in the packed time-major
// layout: frame t of the utterance with length rank r is row rowbase[t] + r.  The K-fold buffer gives every such row S
// slots -- the K hypothesis ranks and, with a reference term, the reference label row -- at row (rowbase[t] + r) * S + s,
// row stride A floats: a batch of ctc_run_batch as it stands (rowbase_S[t] = rowbase[t] * S, frame_off = r * S + s), and
// the S * A floats of one frame are contiguous, so a wave reads whole lines at every A (ctc_mwer.hip's reasoning; a
// padded stride would double the traffic at A = 33 for nothing).  Around that call, none with atomics or a wait for
// another workgroup:
//
//   brnn_mwer_spread_kernel   the probabilities of a row, read once, stored to the slots the row owns: ranks < K_b and
//                             the reference slot.  Other slots are neither read nor written.
//   brnn_mwer_empty_kernel    one wave per slot.  A hypothesis without labels (sctc_ctc_loss_batch rejects U == 0):
//                             cost -sum_t log p[t, blank] in ascending t, rows p - onehot(blank), skip and +inf when a
//                             p_blank is 0.  The other slots: the cost and skip flag of the slot's row in the CTC batch,
//                             or skip = 1 for a slot that is not read -- so that ctc_mwer_coef_kernel sees [B * K].
//   brnn_mwer_combine_kernel  dlogits[row][c] = sum over the real k, ascending, of coef_k * (p - g_k), then ctc_weight *
//                             g_ref, float64, rounded once; +0.0 where nothing contributes.  By select: no row of a
//                             slot that is not real is read; p is read once, from the first real slot.
//   brnn_mwer_results_kernel  the per-utterance results from rank order to caller order.
//
// Lane mapping of spread and combine: a wave takes 64 / G consecutive (t, r), G = the power of two >= A (64 for wider
// rows), lane -> ((t, r), column) by shift and mask, ctc_mwer_combine_kernel's.  Work item i is (t, r) = (i / B, i % B):
// the items with r >= nact[t] (shorter utterances) are idle; an equal-length minibatch has none.
#include <algorithm>
#include <cmath>

#include "brnn_mwer.h"
#include "brnn_mwer_plan.h"
#include "xlane.h"

namespace sctc {
namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_MAX_BLOCKS = 256 * 32;

__global__ __launch_bounds__(BM_THREADS) void brnn_mwer_spread_kernel(BrnnMwerArgs p, int shift, int64_t items)
{
    const int A = p.A, K = p.K, S = p.S, G = 1 << shift;
    const unsigned B = (unsigned)p.B;
    const int lane = threadIdx.x & 63;
    const int sub = lane >> shift, c0 = lane & (G - 1), rpw = 64 >> shift;
    const int64_t step = (int64_t)gridDim.x * (BM_THREADS / 64) * rpw;
    for (int64_t i = ((int64_t)blockIdx.x * (BM_THREADS / 64) + (threadIdx.x >> 6)) * rpw + sub; i < items; i += step) {
        const unsigned t = (unsigned)(i / B), r = (unsigned)(i - (int64_t)t * B);
        if ((int)t >= p.Ts[r]) continue;
        const int64_t row = (int64_t)p.rowbase[t] + r;
        const int kn = min(max(p.kb[r], 0), K);
        const float* src = p.probs + row * p.ld;
        float* dst = p.kprobs + row * S * A;
        for (int c = c0; c < A; c += G) {
            const float v = src[c];
            for (int k = 0; k < kn; ++k) dst[(int64_t)k * A + c] = v;
            if (S > K) dst[(int64_t)K * A + c] = v;
        }
    }
}

__global__ __launch_bounds__(64) void brnn_mwer_empty_kernel(BrnnMwerArgs p)
{
    const int lane = threadIdx.x;
    const int slot = blockIdx.x;                 // r * S + s
    const int S = p.S, K = p.K, A = p.A;
    const int r = slot / S, s = slot - r * S;
    const int src = __builtin_amdgcn_readfirstlane(p.src[slot]);
    double cost = 0.0;
    int skip = 1;
    if (src >= 0) {
        cost = p.ctc_cost[src];
        skip = p.ctc_skip[src];
    } else if (src == BRNN_MWER_SRC_EMPTY) {
        const int T = __builtin_amdgcn_readfirstlane(p.Ts[r]);
        const float* pr = p.kprobs;
        float* gr = p.kgrad;
        double acc = 0.0;
        bool zero = false;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            double lv = 0.0;
            if (t < T) {
                const double pb = (double)pr[((int64_t)p.rowbase_S[t] + slot) * A];
                zero = zero || pb == 0.0;
                lv = log(pb);
            }
            const int cnt = min(64, T - t0);
            for (int i = 0; i < cnt; ++i) acc += __shfl(lv, i, 64);     // ascending t, whatever the lane count
        }
        for (int t = 0; t < T; ++t) {
            const int64_t base = ((int64_t)p.rowbase_S[t] + slot) * A;
            for (int c = lane; c < A; c += 64) gr[base + c] = pr[base + c] - (c == 0 ? 1.0f : 0.0f);
        }
        const bool any_zero = __ballot(zero) != 0ull;
        cost = any_zero ? (double)INFINITY : -acc;
        skip = any_zero ? 1 : 0;
    }
    if (lane == 0) {
        if (s < K) {
            p.cost[(int64_t)r * K + s] = cost;
            p.skip[(int64_t)r * K + s] = skip;
        } else {
            p.ref_cost[r] = cost;
            p.ref_skip[r] = skip;
        }
    }
}

__global__ __launch_bounds__(BM_THREADS) void brnn_mwer_combine_kernel(BrnnMwerArgs p, int shift, int64_t items)
{
#pragma clang fp contract(off)
    const int A = p.A, K = p.K, S = p.S, G = 1 << shift;
    const unsigned B = (unsigned)p.B;
    const int lane = threadIdx.x & 63;
    const int sub = lane >> shift, c0 = lane & (G - 1), rpw = 64 >> shift;
    const int64_t step = (int64_t)gridDim.x * (BM_THREADS / 64) * rpw;
    for (int64_t i = ((int64_t)blockIdx.x * (BM_THREADS / 64) + (threadIdx.x >> 6)) * rpw + sub; i < items; i += step) {
        const unsigned t = (unsigned)(i / B), r = (unsigned)(i - (int64_t)t * B);
        if ((int)t >= p.Ts[r]) continue;
        const int64_t row = (int64_t)p.rowbase[t] + r;
        const int64_t base = row * S * A;
        const bool active = p.inactive[r] == 0;
        const bool ref = S > K && p.ref_skip[r] == 0 && isfinite(p.ref_cost[r]);
        const double* coef = p.coef + (int64_t)r * K;
        const int32_t* real = p.real + (int64_t)r * K;
        int first = 0;
        if (active)
            while (first < K - 1 && !real[first]) ++first;     // an active utterance has a real rank
        float* out = p.dlogits + row * p.ld;
        for (int c = c0; c < A; c += G) {
            double acc = 0.0;
            if (active) {
                const double pv = (double)p.kprobs[base + (int64_t)first * A + c];
                for (int k = 0; k < K; ++k)
                    if (real[k]) acc += coef[k] * (pv - (double)p.kgrad[base + (int64_t)k * A + c]);
            }
            if (ref) acc += p.ctc_weight * (double)p.kgrad[base + (int64_t)K * A + c];
            out[c] = (active || ref) ? (float)acc : 0.0f;
        }
    }
}

__global__ void brnn_mwer_results_kernel(BrnnMwerResults p)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int K = p.K;
    if (i >= p.B * K) return;
    const int r = i / K, k = i - r * K;
    const int b = p.perm[r];
    p.out_post[(int64_t)b * K + k] = p.post[i];
    p.out_real[(int64_t)b * K + k] = p.real[i];
    if (k == 0) {
        double loss = p.loss[r], cc = 0.0;
        int cs = 0;
        if (p.with_ref) {
            cc = p.ref_cost[r];
            cs = (p.ref_skip[r] != 0 || !isfinite(cc)) ? 1 : 0;      // 1: the reference row contributes nothing
            if (cs == 0) loss += p.ctc_weight * cc;
        }
        p.out_loss[b] = loss;
        p.out_expected[b] = p.expected[r];
        p.out_inactive[b] = p.inactive[r];
        p.out_ctc_cost[b] = cc;
        p.out_ctc_skip[b] = cs;
    }
}

int row_shift(int A)
{
    int shift = 0;
    while (shift < 6 && (1 << shift) < A) ++shift;
    return shift;
}

unsigned row_grid(int64_t items, int shift)
{
    const int64_t per_block = (int64_t)(BM_THREADS / 64) * (64 >> shift);
    return (unsigned)std::min<int64_t>((items + per_block - 1) / per_block, BM_MAX_BLOCKS);
}

}  // namespace

int launch_brnn_mwer_spread(const BrnnMwerArgs& a, hipStream_t s)
{
    const int64_t items = (int64_t)a.Tmax * a.B;
    if (items == 0) return SCTC_OK;
    const int shift = row_shift(a.A);
    hipLaunchKernelGGL(brnn_mwer_spread_kernel, dim3(row_grid(items, shift)), dim3(BM_THREADS), 0, s, a, shift, items);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

int launch_brnn_mwer_empty(const BrnnMwerArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(brnn_mwer_empty_kernel, dim3((unsigned)(a.B * a.S)), dim3(64), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

int launch_brnn_mwer_combine(const BrnnMwerArgs& a, hipStream_t s)
{
    const int64_t items = (int64_t)a.Tmax * a.B;
    if (items == 0) return SCTC_OK;
    const int shift = row_shift(a.A);
    hipLaunchKernelGGL(brnn_mwer_combine_kernel, dim3(row_grid(items, shift)), dim3(BM_THREADS), 0, s, a, shift, items);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

int launch_brnn_mwer_results(const BrnnMwerResults& a, hipStream_t s)
{
    const int n = a.B * a.K;
    hipLaunchKernelGGL(brnn_mwer_results_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // namespace sctc
