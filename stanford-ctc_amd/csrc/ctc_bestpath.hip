// Best-path (greedy) CTC decoding of a packed batch in one launch: the per-frame arg-max of
// ctc_fast.pyx:154-187 and new_decoder/decoder.pyx:79-100, the collapse of repeats with a set of symbols that
// are never emitted, the frames of every label and the sum of the arg-max values.  The contract is stated in
// include/sctc.h and restated in NumPy in tests/bestpath_model.py.  Also here: the element-wise logarithm that
// turns the network's probabilities into the decoders' input without leaving the device.
//
// One workgroup of 256 threads per utterance; it walks the utterance in blocks of FB = 256 frames.  Per block:
//   1. best[t] and the row maximum of the block's rows go to LDS, by one of two row-to-lane mappings:
//        lane (A <= LANE_MAX_A = 4096): a row per lane, a serial scan of the row, no cross-lane traffic: 256 rows
//        in flight per workgroup;
//        wave (A > 4096): a row per wave, lane k takes columns k, k + 64, ...; six xor-shuffle steps per row.  A
//        wave owns 64 consecutive rows of the block and has four of them in flight.
//      Measured (profiles/bestpath.md), the row per lane is 6 to 12 times faster at every alphabet from 16 to 4096
//      symbols and runs at memory bandwidth from 256 utterances on; the switch stands at the end of that range.
//      The loads are issued unconditionally with the row index clamped to T - 1 (and the column to A - 1), so no
//      load sits behind a bounds check.
//   2. thread i owns frame t0 + i.  Its left neighbour's best comes from LDS; thread 0's comes from a register
//      that carries the last best of the previous block.  emit = (t == 0 or best != prev) and best not dropped.
//   3. the emitting frames are compacted: a 64-bit __ballot per wave, the population count below the lane, the
//      counts of the waves in front (LDS) and a running offset carried in a register.  The emitting frame writes
//      its label and the span's first frame.
// A span's last frame is written by the frame that ENDS the run, the first frame t with best[t] != best[t-1]:
// the run it closes is the last label emitted before t, at index (labels emitted before t) - 1, wherever its first
// frame was -- in this block, or many blocks earlier; nothing about an open run is kept but the running offset.
// The run that is open at the end of the utterance is closed by thread 0 after the last block.
// Every thread adds the row maxima of its own frames in float64; the 256 partial sums are added by a fixed tree, so
// the score does not depend on the mapping.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"

namespace sctc {
namespace {

constexpr int BP_THREADS = 256;
constexpr int BP_FB = 256;           // frames per block: one per thread
constexpr int BP_LANE_MAX_A = 4096;  // largest alphabet of the row-per-lane mapping (the largest one measured)
constexpr int BP_MAX_DROP = 16;

struct BestUtt {
    int64_t frame_off;      // first row of the utterance
    int64_t out_off;        // sum of T over the utterances in front: where its labels go
    int32_t T;
    int32_t b;
};

struct BestArgs {
    const BestUtt* utts;    // pinned host memory, read once per workgroup
    const void* y;
    int32_t* ids;
    int32_t* lens;
    int32_t* spans;         // may be null
    double* scores;         // may be null
    int64_t ld;
    int32_t A, n_drop;
    int32_t drop[BP_MAX_DROP];
};

template <typename Y, bool PER_WAVE>
__global__ __launch_bounds__(BP_THREADS) void ctc_bestpath_kernel(BestArgs p)
{
    __shared__ int32_t best_s[BP_FB];
    __shared__ double val_s[BP_FB];
    __shared__ int32_t cnt_s[BP_THREADS / 64];
    __shared__ double sum_s[BP_THREADS / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BestUtt d = p.utts[blockIdx.x];
    const int T = __builtin_amdgcn_readfirstlane(d.T);
    const int A = p.A;
    const int64_t ld = p.ld;
    const Y* y = (const Y*)p.y + d.frame_off * ld;
    int32_t* ids = p.ids + d.out_off;
    int32_t* spans = p.spans ? p.spans + 2 * d.out_off : nullptr;

    auto dropped = [&](int v) {
        bool r = false;
#pragma unroll
        for (int i = 0; i < BP_MAX_DROP; ++i) r = r || (i < p.n_drop && v == p.drop[i]);
        return r;
    };

    int carry = -1;         // best of the frame in front of the block; frame 0 has none
    int out = 0;            // labels emitted by the blocks in front
    double acc = 0.0;

    for (int t0 = 0; t0 < T; t0 += BP_FB) {
        // 1. arg-max and maximum of the block's rows
        if constexpr (!PER_WAVE) {
            const int t = min(t0 + tid, T - 1);
            const Y* yr = y + (int64_t)t * ld;
            Y bv = -INFINITY;
            int bi = 0;
#pragma unroll 8
            for (int k = 0; k < A; ++k) {
                const Y v = yr[k];
                if (v > bv) { bv = v; bi = k; }     // the first maximum wins; a row of -inf keeps 0
            }
            best_s[tid] = bi;
            val_s[tid] = (double)bv;
        } else {
            constexpr int RU = 4;                   // rows in flight per wave
            for (int j = 0; j < 64; j += RU) {
                if (t0 + wave * 64 + j >= T) break;     // wave-uniform: the rest of this wave's rows lie beyond the end
                Y bv[RU];
                int bi[RU];
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    const int t = min(t0 + wave * 64 + j + u, T - 1);
                    const Y* yr = y + (int64_t)t * ld;
                    bv[u] = -INFINITY;
                    bi[u] = 0x7fffffff;
                    for (int k0 = 0; k0 < A; k0 += 64) {
                        const int k = k0 + lane;
                        const Y v = yr[min(k, A - 1)];
                        if (k < A && v > bv[u]) { bv[u] = v; bi[u] = k; }
                    }
                }
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    for (int off = 32; off > 0; off >>= 1) {
                        const Y ov = __shfl_xor(bv[u], off, 64);
                        const int oi = __shfl_xor(bi[u], off, 64);
                        if (ov > bv[u] || (ov == bv[u] && oi < bi[u])) { bv[u] = ov; bi[u] = oi; }
                    }
                    if (lane == 0) {
                        best_s[wave * 64 + j + u] = bi[u] == 0x7fffffff ? 0 : bi[u];
                        val_s[wave * 64 + j + u] = (double)bv[u];
                    }
                }
            }
        }
        __syncthreads();

        // 2. the frame of this thread
        const int t = t0 + tid;
        const bool live = t < T;
        const int mine = best_s[tid];
        const int prev = tid == 0 ? carry : best_s[tid - 1];
        const bool starts = live && (t == 0 || mine != prev);
        const bool emit = starts && !dropped(mine);
        const bool closes = starts && t > 0 && !dropped(prev);
        if (live) acc += val_s[tid];
        const int last_live = min(T - t0, BP_FB) - 1;
        const int next_carry = best_s[last_live];

        // 3. compaction
        const unsigned long long ball = __ballot(emit);
        if (lane == 0) cnt_s[wave] = __popcll(ball);
        __syncthreads();
        int before = out + __popcll(ball & ((1ull << lane) - 1ull));
        int total = 0;
#pragma unroll
        for (int w = 0; w < BP_THREADS / 64; ++w) {
            const int c = cnt_s[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (closes && spans) spans[2 * (int64_t)(before - 1) + 1] = t - 1;
        if (emit) {
            ids[before] = mine;
            if (spans) spans[2 * (int64_t)before] = t;
        }
        out += total;
        carry = next_carry;
        __syncthreads();        // best_s / val_s / cnt_s are rewritten by the next block
    }

    if (tid == 0) {
        if (T > 0 && spans && !dropped(carry)) spans[2 * (int64_t)(out - 1) + 1] = T - 1;
        p.lens[d.b] = out;
    }
    if (p.scores) {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) sum_s[wave] = acc;
        __syncthreads();
        if (tid == 0) p.scores[d.b] = (sum_s[0] + sum_s[1]) + (sum_s[2] + sum_s[3]);
    }
}

__global__ __launch_bounds__(256) void log_rows_kernel(const float* __restrict__ probs, float* __restrict__ logp,
                                                       int64_t rows, int A, int64_t ld)
{
    // probs and logp may be the same buffer: an element is read and written by one thread only
    const int64_t n = rows * A;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const int64_t e = ld == A ? i : (i / A) * ld + i % A;
        logp[e] = (float)log((double)probs[e]);
    }
}

template <typename Y>
int launch_bestpath(const BestArgs& a, int B, bool per_wave, hipStream_t s)
{
    if (per_wave)
        hipLaunchKernelGGL((ctc_bestpath_kernel<Y, true>), dim3((unsigned)B), dim3(BP_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((ctc_bestpath_kernel<Y, false>), dim3((unsigned)B), dim3(BP_THREADS), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_ctc_bestpath_batch(const sctc_bestpath_config* cfg, const void* rows_dev, int32_t* ids_dev, int32_t* lens_dev,
                            int32_t* spans_dev, double* scores_dev, void* stream)
{
    SCTC_CHECK_ARG(cfg, "bestpath: null config");
    SCTC_CHECK_ARG(ids_dev && lens_dev, "bestpath: null ids / lens");
    SCTC_CHECK_ARG(cfg->B >= 0, "bestpath: %d utterances", cfg->B);
    SCTC_CHECK_ARG(cfg->A >= 1, "bestpath: alphabet of %d symbols", cfg->A);
    SCTC_CHECK_ARG(cfg->dtype == SCTC_F32 || cfg->dtype == SCTC_F64, "bestpath: dtype %d is neither SCTC_F32 nor SCTC_F64",
                   cfg->dtype);
    SCTC_CHECK_ARG(cfg->n_drop >= 0 && cfg->n_drop <= BP_MAX_DROP, "bestpath: %d dropped symbols, outside 0..%d", cfg->n_drop,
                   BP_MAX_DROP);
    SCTC_CHECK_ARG(cfg->ld >= cfg->A, "bestpath: ld %lld < A %d", (long long)cfg->ld, cfg->A);
    bool per_wave = cfg->A > BP_LANE_MAX_A;
    const char* force = getenv("SCTC_BESTPATH_MAP");
    if (force && *force) {
        if (!strcmp(force, "wave")) per_wave = true;
        else if (!strcmp(force, "lane")) per_wave = false;
        else SCTC_CHECK_ARG(false, "bestpath: SCTC_BESTPATH_MAP=%s is neither lane nor wave", force);
    }
    if (cfg->B == 0) return SCTC_OK;
    SCTC_CHECK_ARG(cfg->T_b && cfg->frame_off, "bestpath: null length / offset array");
    std::vector<BestUtt> utts((size_t)cfg->B);
    int64_t out_off = 0;
    for (int b = 0; b < cfg->B; ++b) {
        SCTC_CHECK_ARG(cfg->T_b[b] >= 0, "bestpath: utterance %d has %d frames", b, cfg->T_b[b]);
        SCTC_CHECK_ARG(cfg->frame_off[b] >= 0, "bestpath: utterance %d has a negative offset", b);
        utts[b].frame_off = cfg->frame_off[b];
        utts[b].out_off = out_off;
        utts[b].T = cfg->T_b[b];
        utts[b].b = b;
        out_off += cfg->T_b[b];
    }
    SCTC_CHECK_ARG(rows_dev || out_off == 0, "bestpath: null rows");
    hipStream_t s = (hipStream_t)stream;
    // the descriptors stay in pinned host memory and every workgroup reads its own once (edit_distance.hip)
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t bytes = utts.size() * sizeof(BestUtt);
    void* pin = stage->acquire(bytes);
    if (!pin) return set_error(SCTC_ERR_HIP, "bestpath: no pinned host memory for %zu bytes of utterance descriptors", bytes);
    memcpy(pin, utts.data(), bytes);
    void* pin_dev = nullptr;
    SCTC_HIP_TRY(hipHostGetDevicePointer(&pin_dev, pin, 0));
    BestArgs a{};
    a.utts = (const BestUtt*)pin_dev;
    a.y = rows_dev;
    a.ids = ids_dev;
    a.lens = lens_dev;
    a.spans = spans_dev;
    a.scores = scores_dev;
    a.ld = cfg->ld;
    a.A = cfg->A;
    a.n_drop = cfg->n_drop;
    for (int i = 0; i < cfg->n_drop; ++i) a.drop[i] = cfg->drop[i];
    PinnedUploadGuard guard(s, true);
    if (cfg->dtype == SCTC_F64) SCTC_TRY(launch_bestpath<double>(a, cfg->B, per_wave, s));
    else SCTC_TRY(launch_bestpath<float>(a, cfg->B, per_wave, s));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();
    return SCTC_OK;
}

int sctc_log_rows(const float* probs_dev, float* logp_dev, int64_t rows, int32_t A, int64_t ld, void* stream)
{
    SCTC_CHECK_ARG(rows >= 0 && A >= 1 && ld >= A, "log_rows: bad shape (rows %lld, A %d, ld %lld)", (long long)rows, A,
                   (long long)ld);
    if (rows == 0) return SCTC_OK;
    SCTC_CHECK_ARG(probs_dev && logp_dev, "log_rows: null pointer");
    const int64_t n = rows * A;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(log_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, probs_dev, logp_dev, rows, (int)A, ld);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
