// CTC forced alignment and sentence scoring: the best path of a given label row through
// the (T, 2U+1) lattice of ctc_fast.pyx:42-76, and optionally the sum over all of its paths, for a packed
// batch of utterances in one launch.  The contract is stated in include/sctc.h and restated in NumPy in
// tests/align_model.py; the Viterbi score is a plain chain of float64 additions and is bit-equal to it.
//
// One workgroup per utterance.  A thread owns SPL consecutive states of the extended row and keeps their
// values in registers for the whole utterance; only the two values at the upper edge of its states travel:
//   wave path (S <= 512): one wave64, SPL = 1, 2, 4 or 8, the edge comes from lane - 1 with one DPP shift
//     (xlane.h; the shift hands lane 0 a 0, which is probability 1 in the log domain, so lane 0 replaces it
//     with -inf);
//   wide path (S <= 8191): up to 1024 threads, SPL = 8, the edge goes through a double-buffered LDS array,
//     one barrier per frame.
// The symbol column and the skip permission of a state are worked out once per utterance.  The loads of
// y_t(x[s]) are issued PF frames ahead into a register ring, unconditionally (the frame index is clamped),
// so no load waits behind the frame it is needed in.  The recursion starts from a virtual frame -1 that
// holds -0.0 in state 0 and -inf elsewhere: -0.0 + y = y exactly, so frame 0 needs no code of its own.
//
// Back-pointers are 2 bits per state and frame (0 stay, 1 from s-1, 2 from s-2).  A thread packs those of
// its SPL states over FPW = 16 / SPL frames into one 32-bit word: word (t / FPW) * NL + thread.  The words
// stay in LDS when they fit BP_LDS_BYTES, otherwise they go to a slice of the caller's workspace.  The
// trace-back is one thread's walk over LDS: workspace words are first staged into LDS, STAGE_BYTES at a
// time, with coalesced loads by all threads.  The walk writes frame_label and the spans.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "xlane.h"

namespace sctc {
namespace {

constexpr int ALIGN_MAX_U = 4095;
constexpr int WAVE_MAX_S = 512;             // 64 lanes x 8 states
constexpr int WIDE_SPL = 8;
constexpr int HEAD_BYTES = 64;              // the four end values
constexpr size_t BP_LDS_BYTES = 64 * 1024;  // back-pointer words of an utterance stay in LDS up to this size
constexpr size_t STAGE_BYTES = 16 * 1024;   // otherwise: LDS block that the trace-back stages them through

struct AlignUtt {
    int64_t frame_off, label_off, span_off;
    int64_t bp_off;         // bytes into the workspace when the back-pointers are not in LDS
    int32_t T, U;
    int32_t b;              // index of the utterance in the caller's order
    int32_t bp_lds;
};

struct AlignArgs {
    const AlignUtt* utts;   // pinned host memory, read once per workgroup
    const void* y;
    const int32_t* labels;
    int32_t* frame_label;
    int32_t* span;
    double* scores;
    int32_t* status;
    char* ws;
    int32_t A, blank, ld;
};

__device__ __forceinline__ double shr1_ninf(double v, int lane)
{
    const double r = lane_shr1(v);
    return lane == 0 ? -INFINITY : r;
}

__device__ __forceinline__ double lse2(double a, double b)     // the combine of ctc_beam.hip
{
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m));
}
__device__ __forceinline__ double lse3(double a, double b, double c)
{
    const double m = fmax(fmax(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

template <typename Y, int SPL, bool WIDE, bool TOTAL>
__global__ __launch_bounds__(WIDE ? 1024 : 64) void ctc_align_kernel(AlignArgs p)
{
    extern __shared__ __align__(16) char align_lds[];
    constexpr int FPW = 16 / SPL;           // frames per back-pointer word
    constexpr int PF = WIDE ? 2 : 4;        // frames of loads in flight
    const int tid = threadIdx.x;
    const int NL = WIDE ? (int)blockDim.x : 64;
    const AlignUtt d = p.utts[blockIdx.x];
    const int T = __builtin_amdgcn_readfirstlane(d.T), U = __builtin_amdgcn_readfirstlane(d.U);
    const int bp_lds = __builtin_amdgcn_readfirstlane(d.bp_lds);
    const int S = 2 * U + 1;
    const double NINF = -INFINITY;

    double* fin = (double*)align_lds;                               // v(S-1), v(S-2), a(S-1), a(S-2)
    double2* edge = (double2*)(align_lds + HEAD_BYTES);             // wide: [2][NL] (v(last), v(last-1)) of a thread
    double2* edge_a = edge + 2 * NL;                                // wide, total: the same of a
    char* rest = align_lds + HEAD_BYTES + (WIDE ? (size_t)2 * NL * sizeof(double2) * (TOTAL ? 2 : 1) : 0);
    uint32_t* bp = bp_lds ? (uint32_t*)rest : (uint32_t*)(p.ws + d.bp_off);
    uint32_t* stage = (uint32_t*)rest;

    int32_t* fl = p.frame_label + d.frame_off;
    int32_t* sp = p.span + 2 * d.span_off;
    double* sc = p.scores + 2 * (int64_t)d.b;
    int32_t* st = p.status + d.b;

    auto fail = [&](int code) {
        for (int t = tid; t < T; t += NL) fl[t] = -1;
        for (int i = tid; i < 2 * U; i += NL) sp[i] = -1;
        if (tid == 0) {
            sc[0] = NINF;
            sc[1] = TOTAL ? NINF : (double)NAN;
            *st = code;
        }
    };

    if (T == 0) {
        if (U == 0) {
            if (tid == 0) { sc[0] = 0.0; sc[1] = TOTAL ? 0.0 : (double)NAN; *st = 0; }
        } else {
            fail(1);
        }
        return;
    }

    // the symbol column and the skip permission of my states, once per utterance
    const int32_t* lab = p.labels + d.label_off;
    const int s0 = tid * SPL;
    int sym[SPL];
    uint32_t skipm = 0;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = s0 + k;
        sym[k] = p.blank;
        if ((s & 1) && s < S) {
            const int l = lab[(s - 1) >> 1];
            if (l < 0 || l >= p.A || l == p.blank) bad = 1;
            else sym[k] = l;
            if (s >= 3 && lab[(s - 3) >> 1] != l) skipm |= 1u << k;
        }
    }
    if (__syncthreads_or(bad)) {
        fail(2);
        return;
    }

    const Y* y = (const Y*)p.y + d.frame_off * p.ld;
    double yb[PF][SPL];
#pragma unroll
    for (int j = 0; j < PF; ++j) {
        const Y* row = y + (int64_t)min(j, T - 1) * p.ld;
#pragma unroll
        for (int k = 0; k < SPL; ++k) yb[j][k] = (double)row[sym[k]];
    }

    double v[SPL], a[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        v[k] = s0 + k == 0 ? -0.0 : NINF;       // frame -1
        a[k] = v[k];
    }
    if (WIDE) {
        edge[NL + tid] = make_double2(v[SPL - 1], v[SPL - 2 >= 0 ? SPL - 2 : 0]);
        if (TOTAL) edge_a[NL + tid] = make_double2(a[SPL - 1], a[SPL - 2 >= 0 ? SPL - 2 : 0]);
        __syncthreads();
    }

    uint32_t word = 0;
    for (int t0 = 0; t0 < T; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = t0 + j;
            double yv[SPL];
            {
                const Y* row = y + (int64_t)min(t + PF, T - 1) * p.ld;
#pragma unroll
                for (int k = 0; k < SPL; ++k) {
                    yv[k] = yb[j][k];
                    yb[j][k] = (double)row[sym[k]];
                }
            }
            if (t < T) {
                double l1, l2, al1 = NINF, al2 = NINF;          // states s0 - 1 and s0 - 2
                if (WIDE) {
                    const int rb = ((t + 1) & 1) * NL;
                    if (tid) {
                        const double2 e = edge[rb + tid - 1];
                        l1 = e.x; l2 = e.y;
                        if (TOTAL) { const double2 ea = edge_a[rb + tid - 1]; al1 = ea.x; al2 = ea.y; }
                    } else {
                        l1 = NINF; l2 = NINF;
                    }
                } else {
                    l1 = shr1_ninf(v[SPL - 1], tid);
                    l2 = SPL >= 2 ? shr1_ninf(v[SPL >= 2 ? SPL - 2 : 0], tid) : shr1_ninf(l1, tid);
                    if (TOTAL) {
                        al1 = shr1_ninf(a[SPL - 1], tid);
                        al2 = SPL >= 2 ? shr1_ninf(a[SPL >= 2 ? SPL - 2 : 0], tid) : shr1_ninf(al1, tid);
                    }
                }
                uint32_t bits = 0;
#pragma unroll
                for (int k = SPL - 1; k >= 0; --k) {            // downwards: v[k-1], v[k-2] are still frame t-1
                    const bool skip = (skipm >> k) & 1;
                    const double c0 = v[k];
                    const double c1 = k >= 1 ? v[k >= 1 ? k - 1 : 0] : l1;
                    double c2 = k >= 2 ? v[k >= 2 ? k - 2 : 0] : (k == 1 ? l1 : l2);
                    c2 = skip ? c2 : NINF;
                    double m = c0;
                    uint32_t q = 0;
                    if (c1 > m) { m = c1; q = 1; }              // ties: the first of (stay, s-1, s-2)
                    if (c2 > m) { m = c2; q = 2; }
                    v[k] = m + yv[k];
                    bits |= q << (2 * k);
                    if (TOTAL) {
                        const double a1 = k >= 1 ? a[k >= 1 ? k - 1 : 0] : al1;
                        double a2 = k >= 2 ? a[k >= 2 ? k - 2 : 0] : (k == 1 ? al1 : al2);
                        a2 = skip ? a2 : NINF;
                        a[k] = lse3(a[k], a1, a2) + yv[k];
                    }
                }
                const int f = t % FPW;
                word |= bits << (2 * SPL * f);
                if (f == FPW - 1 || t == T - 1) {
                    bp[(size_t)(t / FPW) * NL + tid] = word;
                    word = 0;
                }
                if (WIDE) {
                    const int wb = (t & 1) * NL;
                    edge[wb + tid] = make_double2(v[SPL - 1], v[SPL >= 2 ? SPL - 2 : 0]);
                    if (TOTAL) edge_a[wb + tid] = make_double2(a[SPL - 1], a[SPL >= 2 ? SPL - 2 : 0]);
                    __syncthreads();
                }
            }
        }
    }

    // the end: state S-1, unless S-2 is strictly better
    if (tid == 0 && S == 1) { fin[1] = NINF; fin[3] = NINF; }
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int s = s0 + k;
        if (s == S - 1) { fin[0] = v[k]; fin[2] = TOTAL ? a[k] : NINF; }
        if (s == S - 2) { fin[1] = v[k]; fin[3] = TOTAL ? a[k] : NINF; }
    }
    __threadfence();                // the back-pointer words in the workspace, before other threads read them
    __syncthreads();
    const double vend = fin[0], vpen = fin[1];
    const bool pen = vpen > vend;
    const double vit = pen ? vpen : vend;
    if (!(vit > NINF)) {
        fail(1);
        return;
    }
    if (tid == 0) {
        sc[0] = vit;
        sc[1] = TOTAL ? lse2(fin[2], fin[3]) : (double)NAN;
        *st = 0;
    }

    // trace-back: thread 0 walks LDS, block by block when the words had to go to the workspace
    const int rows = (T + FPW - 1) / FPW;
    const int rows_blk = bp_lds ? rows : (int)(STAGE_BYTES / ((size_t)NL * sizeof(uint32_t)));
    int s = pen ? S - 2 : S - 1, s_next = -1;
    for (int r_hi = rows; r_hi > 0; r_hi -= rows_blk) {
        const int r_lo = max(0, r_hi - rows_blk);
        const uint32_t* w = bp;
        if (!bp_lds) {
            const int n = (r_hi - r_lo) * NL;
            const uint32_t* src = bp + (size_t)r_lo * NL;
            for (int i = tid; i < n; i += NL) stage[i] = src[i];
            __syncthreads();
            w = stage;
        }
        const int r_base = bp_lds ? 0 : r_lo;
        if (tid == 0) {
            for (int t = min(T, r_hi * FPW) - 1; t >= r_lo * FPW; --t) {
                const uint32_t ww = w[(size_t)(t / FPW - r_base) * NL + s / SPL];
                const int q = t > 0 ? (ww >> (2 * (SPL * (t % FPW) + s % SPL))) & 3 : 0;
                const int s_prev = max(s - q, 0);               // a path of finite score never leaves the row
                const int u = (s - 1) >> 1;
                if (s & 1) {
                    fl[t] = u;
                    if (s_next != s) sp[2 * u + 1] = t;
                    if (t == 0 || s_prev != s) sp[2 * u] = t;
                } else {
                    fl[t] = -1;
                }
                s_next = s;
                s = s_prev;
            }
        }
        if (!bp_lds) __syncthreads();
    }
}

struct AlignPlan {
    std::vector<AlignUtt> utts;
    int spl = 1, nl = 64;
    bool wide = false;
    size_t lds = 0, ws_bytes = 0;
    bool any_frames = false, any_labels = false;
};

int plan_align(const sctc_align_config* cfg, AlignPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "align: null config");
    SCTC_CHECK_ARG(cfg->B >= 0, "align: %d utterances", cfg->B);
    SCTC_CHECK_ARG(cfg->A >= 1, "align: alphabet of %d symbols", cfg->A);
    SCTC_CHECK_ARG(cfg->dtype == SCTC_F32 || cfg->dtype == SCTC_F64, "align: dtype %d is neither SCTC_F32 nor SCTC_F64", cfg->dtype);
    SCTC_CHECK_ARG(cfg->blank >= 0 && cfg->blank < cfg->A, "align: blank %d outside [0, %d)", cfg->blank, cfg->A);
    SCTC_CHECK_ARG(cfg->ld >= cfg->A, "align: ld %d < A %d", cfg->ld, cfg->A);
    SCTC_CHECK_ARG((cfg->flags & ~SCTC_ALIGN_TOTAL) == 0, "align: unknown flags 0x%x", cfg->flags);
    if (cfg->B == 0) return SCTC_OK;
    SCTC_CHECK_ARG(cfg->T_b && cfg->frame_off && cfg->U_b && cfg->label_off, "align: null length / offset array");
    int umax = 0;
    for (int b = 0; b < cfg->B; ++b) {
        SCTC_CHECK_ARG(cfg->T_b[b] >= 0, "align: utterance %d has %d frames", b, cfg->T_b[b]);
        SCTC_CHECK_ARG(cfg->U_b[b] >= 0 && cfg->U_b[b] <= ALIGN_MAX_U, "align: utterance %d has %d labels, outside 0..%d", b,
                       cfg->U_b[b], ALIGN_MAX_U);
        SCTC_CHECK_ARG(cfg->frame_off[b] >= 0 && cfg->label_off[b] >= 0, "align: utterance %d has a negative offset", b);
        umax = std::max(umax, cfg->U_b[b]);
    }
    // one path for the batch, chosen by its longest label row (as the CTC loss paths are)
    const int smax = 2 * umax + 1;
    const char* force = getenv("SCTC_ALIGN_PATH");
    pl.wide = smax > WAVE_MAX_S;
    if (force && *force) {
        if (!strcmp(force, "wide")) pl.wide = true;
        else if (!strcmp(force, "wave")) {
            SCTC_CHECK_ARG(smax <= WAVE_MAX_S, "align: SCTC_ALIGN_PATH=wave with %d states, the wave path holds %d", smax, WAVE_MAX_S);
        } else {
            SCTC_CHECK_ARG(false, "align: SCTC_ALIGN_PATH=%s is neither wave nor wide", force);
        }
    }
    if (pl.wide) {
        pl.spl = WIDE_SPL;
        pl.nl = (int)round_up((smax + WIDE_SPL - 1) / WIDE_SPL, 64);
    } else {
        pl.spl = smax <= 64 ? 1 : smax <= 128 ? 2 : smax <= 256 ? 4 : 8;
        pl.nl = 64;
    }
    const bool total = (cfg->flags & SCTC_ALIGN_TOTAL) != 0;
    const int fpw = 16 / pl.spl;
    size_t rest = 0;
    int64_t span_off = 0;
    pl.utts.reserve(cfg->B);
    for (int b = 0; b < cfg->B; ++b) {
        AlignUtt d{};
        d.frame_off = cfg->frame_off[b];
        d.label_off = cfg->label_off[b];
        d.span_off = span_off;
        d.T = cfg->T_b[b];
        d.U = cfg->U_b[b];
        d.b = b;
        span_off += d.U;
        pl.any_frames |= d.T > 0;
        pl.any_labels |= d.U > 0;
        const size_t bp_b = (size_t)((d.T + fpw - 1) / fpw) * pl.nl * sizeof(uint32_t);
        if (bp_b <= BP_LDS_BYTES) {
            d.bp_lds = 1;
            rest = std::max(rest, bp_b);
        } else {
            d.bp_off = (int64_t)pl.ws_bytes;
            pl.ws_bytes += align256(bp_b);
            rest = std::max(rest, STAGE_BYTES);
        }
        pl.utts.push_back(d);
    }
    pl.lds = HEAD_BYTES + (pl.wide ? (size_t)2 * pl.nl * sizeof(double2) * (total ? 2 : 1) : 0) + rest;
    return SCTC_OK;
}

template <typename Y, int SPL, bool WIDE, bool TOTAL>
int launch_align(const AlignArgs& a, const AlignPlan& pl, hipStream_t s)
{
    auto kern = &ctc_align_kernel<Y, SPL, WIDE, TOTAL>;
    if (pl.lds > 64 * 1024)
        SCTC_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.utts.size()), dim3(pl.nl), pl.lds, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

template <typename Y, bool TOTAL>
int launch_align_path(const AlignArgs& a, const AlignPlan& pl, hipStream_t s)
{
    if (pl.wide) return launch_align<Y, WIDE_SPL, true, TOTAL>(a, pl, s);
    switch (pl.spl) {
    case 1: return launch_align<Y, 1, false, TOTAL>(a, pl, s);
    case 2: return launch_align<Y, 2, false, TOTAL>(a, pl, s);
    case 4: return launch_align<Y, 4, false, TOTAL>(a, pl, s);
    default: return launch_align<Y, 8, false, TOTAL>(a, pl, s);
    }
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_ctc_align_workspace_bytes(const sctc_align_config* cfg, size_t* bytes)
{
    SCTC_CHECK_ARG(bytes, "align: null bytes");
    *bytes = 0;
    AlignPlan pl;
    SCTC_TRY(plan_align(cfg, pl));
    *bytes = pl.ws_bytes;
    return SCTC_OK;
}

int sctc_ctc_align_batch(const sctc_align_config* cfg, const void* logprobs_dev, const int32_t* labels_dev,
                         int32_t* frame_label_dev, int32_t* span_dev, double* scores_dev, int32_t* status_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream)
{
    AlignPlan pl;
    SCTC_TRY(plan_align(cfg, pl));
    if (cfg->B == 0) return SCTC_OK;
    SCTC_CHECK_ARG(scores_dev && status_dev, "align: null scores / status");
    SCTC_CHECK_ARG((logprobs_dev && frame_label_dev) || !pl.any_frames, "align: null logprobs / frame_label");
    SCTC_CHECK_ARG((labels_dev && span_dev) || !pl.any_labels, "align: null labels / span");
    if (workspace_bytes < pl.ws_bytes || (pl.ws_bytes && !workspace_dev))
        return set_error(SCTC_ERR_WORKSPACE, "align: workspace %zu bytes < %zu needed", workspace_dev ? workspace_bytes : (size_t)0,
                         pl.ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    // the descriptors stay in pinned host memory and every workgroup reads its own once (edit_distance.hip)
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t bytes = pl.utts.size() * sizeof(AlignUtt);
    void* pin = stage->acquire(bytes);
    if (!pin) return set_error(SCTC_ERR_HIP, "align: no pinned host memory for %zu bytes of utterance descriptors", bytes);
    memcpy(pin, pl.utts.data(), bytes);
    void* pin_dev = nullptr;
    SCTC_HIP_TRY(hipHostGetDevicePointer(&pin_dev, pin, 0));
    AlignArgs a{};
    a.utts = (const AlignUtt*)pin_dev;
    a.y = logprobs_dev;
    a.labels = labels_dev;
    a.frame_label = frame_label_dev;
    a.span = span_dev;
    a.scores = scores_dev;
    a.status = status_dev;
    a.ws = (char*)workspace_dev;
    a.A = cfg->A;
    a.blank = cfg->blank;
    a.ld = cfg->ld;
    const bool total = (cfg->flags & SCTC_ALIGN_TOTAL) != 0;
    PinnedUploadGuard guard(s, true);
    if (cfg->dtype == SCTC_F64)
        SCTC_TRY(total ? (launch_align_path<double, true>(a, pl, s)) : (launch_align_path<double, false>(a, pl, s)));
    else
        SCTC_TRY(total ? (launch_align_path<float, true>(a, pl, s)) : (launch_align_path<float, false>(a, pl, s)));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();
    return SCTC_OK;
}

}  // extern "C"
