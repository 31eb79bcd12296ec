// LM scores of label sequences on the device and n-best rescoring: the second pass behind the four
// beam searches.  sctc_lm_score_batch walks N sequences of CTC symbols under one of the three character LMs and keeps,
// of every LM row, only the entry of the label that follows: term i = log10 P_LM(l_i | <s>, l_0 .. l_{i-1}), the
// float32 value the beam search of that LM adds for the extension.
//
//   recurrent LM    one workgroup walks a tile of up to 32 whole sequences in lockstep (lm_score_plan.h orders them by
//                   descending length, so the live slots of a step are a prefix of the tile): step 0 feeds <s> to the
//                   zero state, step i the LM id of l_{i-1}; after each rnnlm_tile call lane e keeps
//                   rows[e * Vp + sym_word[l_i]].  The states alternate between two [32][H] buffers of the tile.
//   window LM       a tile is 32 positions of the flattened list; the kernel builds each window by the rule of
//                   nn_lm.NNCharLM.context_ids (the last K LM ids of the prefix; fewer: null .. null, <s>, ids), calls
//                   nnlm_tile and keeps the target column.
//   n-gram LM       one lane per position: the newest order - 1 LM ids, <s> included while it is in reach, packed
//                   newest in the low byte, and the probe of the beam search.
//
// rnnlm_tile and nnlm_tile are the routines the searches call (rnnlm_dev.h, nnlm_dev.h): a row is the same function of
// the prefix here as there, bit for bit.  One small kernel, shared by the three, adds a sequence's terms in position
// order in float64.  A second entry, sctc_nbest_rank_batch, combines the totals of one forced-alignment launch with the
// LM sums and ranks each utterance's hypotheses, one wave per utterance, by counting; sctc_nbest_rank_words_batch is the
// same kernel instantiated with the word-LM term of word_lm_score.hip (§4.14).
#include <math.h>

#include <vector>

#include "beam_lm.h"
#include "beam_search.h"
#include "common.h"
#include "lm_score_plan.h"
#include "rnnlm_dev.h"

namespace sctc {
namespace {

using beam::AMAX;
using beam::KMAX;
using beam::mix64;

static_assert(LM_SCORE_TILE == NN_TILE, "lm_score_plan.h cuts tiles of nnlm_dev.h's size");

struct LmScoreArgs {
    const LmSeq* seqs;          // workspace
    const LmTile* tiles;
    const int32_t* sym;         // [A]
    const int32_t* labels;
    float* terms;               // the caller's, or the workspace's
    double* sums;
    int32_t* status;
    char* scratch;
    size_t tile_bytes;
    int64_t n_terms, n_tiles;
    int32_t N, A;
};

// ---- status: a label outside [1, A) ------------------------------------------------------------------------------
// one wave per sequence; the path kernels and the sums read what this launch wrote
__global__ __launch_bounds__(256) void lm_status_kernel(LmScoreArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= p.N) return;
    const LmSeq d = p.seqs[idx];
    bool bad = false;
    for (int i = lane; i < d.U; i += 64) {
        const int c = p.labels[d.label_off + i];
        bad |= c <= 0 || c >= p.A;
    }
    const bool any = __any(bad);
    if (lane == 0) p.status[d.n] = any ? 2 : 0;
}

// ---- sums: float64, position order -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lm_sums_kernel(LmScoreArgs p)
{
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.N) return;
    const LmSeq d = p.seqs[idx];
    double s = 0.0;
    if (p.status[d.n] != 0) {
        s = -INFINITY;
    } else {
        const float* t = p.terms + d.term_off;
        for (int i = 0; i < d.U; ++i) s += (double)t[i];
    }
    p.sums[d.n] = s;
}

// the sequence that holds position pos of the flattened list (descriptors in the caller's order, term_off ascending;
// a sequence without labels shares its term_off with its successor and is never the answer)
__device__ __forceinline__ int32_t seq_of_position(const LmSeq* seqs, int32_t N, int64_t pos)
{
    int32_t lo = 0, hi = N;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (seqs[mid].term_off <= pos) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// ---- the n-gram LM -----------------------------------------------------------------------------------------------
// ctc_beam_kernel keeps its instruction stream (beam_ngram.h), so its table probe is not shared from there: lm_find and
// lm_score of that header are restated here over a small table struct, statement for statement.  A change to the
// probe, the order of the back-offs or the packing of the context is made in both files.
struct NgramTab {
    const uint64_t* key;
    const float* prob;
    const float* bo;
    uint64_t mask;
    int32_t order, bos;
};

__device__ inline uint64_t ng_bytes_mask(int m) { return m >= 8 ? ~0ull : ((1ull << (8 * m)) - 1); }

__device__ inline bool ng_find(const NgramTab& p, uint64_t key, float& pr, float& bo)
{
    uint64_t s = mix64(key) & p.mask;
    while (true) {
        const uint64_t k = p.key[s];
        if (k == key) {
            pr = p.prob[s];
            bo = p.bo[s];
            return true;
        }
        if (k == 0) return false;
        s = (s + 1) & p.mask;
    }
}

__device__ float ng_score(const NgramTab& p, uint64_t ctx, int ctxlen, uint32_t w)
{
#pragma clang fp contract(off)
    float pr = -100.0f, bo = 0.0f;
    ng_find(p, w, pr, bo);
    float best = pr;
    int n = 1;
    for (int m = 1; m <= ctxlen; ++m) {
        if (!ng_find(p, ((ctx & ng_bytes_mask(m)) << 8) | w, pr, bo)) break;
        best = pr;
        n = m + 1;
    }
    for (int m = n; m <= ctxlen; ++m) {
        if (!ng_find(p, ctx & ng_bytes_mask(m), pr, bo)) break;
        best = best + bo;
    }
    return best;
}

__global__ __launch_bounds__(LM_SCORE_NGRAM_THREADS) void lm_score_ngram_kernel(LmScoreArgs p, NgramTab tab)
{
    const int ctx_max = tab.order - 1;
    const int64_t stride = (int64_t)gridDim.x * LM_SCORE_NGRAM_THREADS;
    for (int64_t pos = (int64_t)blockIdx.x * LM_SCORE_NGRAM_THREADS + threadIdx.x; pos < p.n_terms; pos += stride) {
        const LmSeq d = p.seqs[seq_of_position(p.seqs, p.N, pos)];
        if (p.status[d.n] != 0) continue;
        const int i = (int)(pos - d.term_off);
        const int32_t* l = p.labels + d.label_off;
        const int ctxlen = min(i + 1, ctx_max);
        uint64_t ctx = 0;
        for (int k = i - ctxlen; k < i; ++k) ctx = (ctx << 8) | (uint64_t)(k < 0 ? tab.bos : p.sym[l[k]]);
        p.terms[pos] = ng_score(tab, ctx, ctxlen, (uint32_t)p.sym[l[i]]);
    }
}

// ---- the window LM -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NN_THREADS) void lm_score_nn_kernel(LmScoreArgs p, NNLMDev m)
{
    const int K = m.K, Vp = m.Vp;
    char* w = p.scratch + (size_t)blockIdx.x * p.tile_bytes;
    float* act = (float*)w;
    float* rows = (float*)(w + nn_act_bytes(m.hmax));
    int32_t* ids = (int32_t*)(w + nn_act_bytes(m.hmax) + nn_row_bytes(Vp));
    const int e = threadIdx.x;
    for (int64_t t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        const int64_t first = t * NN_TILE;
        const int cnt = (int)min((int64_t)NN_TILE, p.n_terms - first);
        int target = -1;
        if (e < cnt) {
            const int64_t pos = first + e;
            const LmSeq d = p.seqs[seq_of_position(p.seqs, p.N, pos)];
            const bool ok = p.status[d.n] == 0;
            const int i = (int)(pos - d.term_off);
            const int32_t* l = p.labels + d.label_off;
            // slot s of the window holds prefix element i - K + s; element -1 is <s>, older ones the null id
            for (int s = 0; s < K; ++s) {
                const int j = i - K + s;
                int id = m.bos;
                if (ok) id = j >= 0 ? p.sym[l[j]] : (j == -1 ? m.bos : m.null_id);
                ids[e * K + s] = id;
            }
            if (ok) target = p.sym[l[i]];
        }
        __syncthreads();
        nnlm_tile(m, ids, cnt, act, rows);
        if (target >= 0) p.terms[first + e] = rows[(size_t)e * Vp + target];
        __syncthreads();
    }
}

// ---- the recurrent LM --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NN_THREADS) void lm_score_rnn_kernel(LmScoreArgs p, RNNLMDev m)
{
    __shared__ int s_cnt;
    const int H = m.H, Vp = m.Vp;
    char* w = p.scratch + (size_t)blockIdx.x * p.tile_bytes;
    float* act = (float*)w;
    float* rows = (float*)(w + nn_act_bytes(H));
    int32_t* slot = (int32_t*)(w + nn_act_bytes(H) + nn_row_bytes(Vp));
    const size_t state_bytes = align256((size_t)NN_TILE * H * sizeof(float));
    float* st[2] = {(float*)(w + rnn_tile_bytes(H, Vp)), (float*)(w + rnn_tile_bytes(H, Vp) + state_bytes)};
    const int e = threadIdx.x;
    for (int64_t t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        const LmTile tl = p.tiles[t];
        int U = 0;
        bool ok = false;
        const int32_t* l = nullptr;
        float* out = nullptr;
        if (e < tl.cnt) {
            const LmSeq d = p.seqs[tl.first + e];
            U = d.U;
            ok = p.status[d.n] == 0;
            l = p.labels + d.label_off;
            out = p.terms + d.term_off;
        }
        int prev = 0;      // l_{step-1} of my sequence
        for (int step = 0; step < tl.steps; ++step) {
            const bool live = U > step;
            if (threadIdx.x < 64) {     // the sequences are in descending length: the live slots are 0 .. cnt-1
                const unsigned long long b = __ballot(live);
                if (threadIdx.x == 0) s_cnt = __popcll(b);
            }
            int cur = 0;
            if (live) {
                cur = l[step];
                // a sequence with a label outside the alphabet (status 2) keeps its slot and feeds <s>
                slot[e] = (step == 0 || !ok) ? m.bos : p.sym[prev];
                slot[NN_TILE + e] = e;
                slot[2 * NN_TILE + e] = e;
            }
            __syncthreads();
            const int cnt = s_cnt;
            rnnlm_tile(m, slot, cnt, step == 0 ? nullptr : st[(step & 1) ^ 1], st[step & 1], act, rows);
            if (live && ok) out[step] = rows[(size_t)e * Vp + p.sym[cur]];
            prev = cur;
            __syncthreads();
        }
    }
}

// ---- combine and rank --------------------------------------------------------------------------------------------
struct RankArgs {
    const int32_t* Kb;      // pinned host [B]
    const int32_t* U;       // pinned host [B * K]
    const double* scores;   // [B * K][2]
    const int32_t* status;
    const double* lm;       // or nullptr
    const double* first;    // or nullptr
    double* out;
    int32_t* order;
    double alpha, beta;
    int32_t B, K;
    // the word-LM term of sctc_nbest_rank_words_batch (§4.14); not read by the kernel without it
    const double* wsum;     // [B * K]
    const int32_t* wcount;  // [B * K][2]: words, OOV words
    const int32_t* wstatus; // [B * K]
    double walpha, wbeta;
};

template <bool WORDS>
__global__ __launch_bounds__(256) void nbest_rank_kernel(RankArgs p)
{
#pragma clang fp contract(off)
    __shared__ double sc[4][KMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= p.B) return;       // whole waves leave; there is no workgroup barrier below
    const int K = p.K;
    int kb = p.Kb[b];
    if (p.first)
        for (int base = 0; base < kb; base += 64) {
            const int k = base + lane;
            const unsigned long long gone = __ballot(k < kb && p.first[b * K + k] == -INFINITY);
            if (gone) {
                kb = base + __ffsll((long long)gone) - 1;
                break;
            }
        }
    double* s = sc[wave];
    for (int k = lane; k < K; k += 64) {
        const int64_t o = b * K + k;
        double v = -INFINITY;
        if (k < kb && p.status[o] == 0) {
            const double lm = p.lm ? p.lm[o] : 0.0;
            const double a = p.alpha * lm;
            const double t = p.scores[2 * o + 1] + a;
            const double bu = p.beta * (double)p.U[o];
            v = t + bu;
            if constexpr (WORDS) {
                // a hypothesis the word LM cannot score is out: no 0 * -inf
                if (p.wstatus[o] == 0) {
                    const double wa = p.walpha * p.wsum[o];
                    const double wb = p.wbeta * (double)p.wcount[2 * o];
                    const double wt = wa + wb;
                    v = v + wt;
                } else {
                    v = -INFINITY;
                }
            }
        }
        s[k] = v;
        p.out[o] = v;
    }
    // every lane reads what every lane of this wave wrote
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (int k = lane; k < K; k += 64) {
        int r = k;              // a rank that is not real keeps its place
        if (k < kb) {
            const double v = s[k];
            r = 0;
            for (int j = 0; j < kb; ++j) {
                const double vj = s[j];
                r += (vj > v) || (vj == v && j < k);
            }
        }
        p.order[b * K + r] = k;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------
struct LmScoreCall {
    LmScorePlan plan;
    size_t tile_bytes = 0;
    int device = -1;
};

int plan_lm_score(const sctc_lm_score_config* cfg, bool terms_in_ws, LmScoreCall& c)
{
    SCTC_CHECK_ARG(cfg, "lm_score: null config");
    SCTC_CHECK_ARG(cfg->N >= 0, "lm_score: %d sequences", cfg->N);
    SCTC_CHECK_ARG(cfg->A >= 1 && cfg->A <= AMAX, "lm_score: alphabet of %d symbols outside 1..%d", cfg->A, AMAX);
    SCTC_CHECK_ARG(cfg->lm_kind == SCTC_LM_NGRAM || cfg->lm_kind == SCTC_LM_NN || cfg->lm_kind == SCTC_LM_RNN,
                   "lm_score: unknown LM kind %d", cfg->lm_kind);
    SCTC_CHECK_ARG(cfg->reserved == 0, "lm_score: reserved field is %d", cfg->reserved);
    SCTC_CHECK_ARG(cfg->lm, "lm_score: null LM");
    SCTC_CHECK_ARG(cfg->sym_word, "lm_score: null symbol map");
    SCTC_CHECK_ARG(cfg->N == 0 || (cfg->U_b && cfg->label_off), "lm_score: null length / offset array");
    for (int n = 0; n < cfg->N; ++n) {
        SCTC_CHECK_ARG(cfg->U_b[n] >= 0 && cfg->U_b[n] <= LM_SCORE_MAX_U, "lm_score: sequence %d has %d labels, outside 0..%d", n,
                       cfg->U_b[n], LM_SCORE_MAX_U);
        SCTC_CHECK_ARG(cfg->label_off[n] >= 0, "lm_score: sequence %d has a negative offset", n);
    }
    // what follows reads the handle
    int lo = 0, hi = 0;
    if (cfg->lm_kind == SCTC_LM_NGRAM) {
        const sctc_lm* lm = (const sctc_lm*)cfg->lm;
        lo = 1;
        hi = 255;
        c.tile_bytes = 0;
        c.device = lm->device;
    } else if (cfg->lm_kind == SCTC_LM_NN) {
        const sctc_nnlm* lm = (const sctc_nnlm*)cfg->lm;
        hi = lm->dev.V - 1;
        c.tile_bytes = nn_tile_bytes(lm->dev.hmax, lm->dev.Vp, lm->dev.K);
        c.device = lm->device;
    } else {
        const sctc_rnnlm* lm = (const sctc_rnnlm*)cfg->lm;
        hi = lm->dev.V - 1;
        c.tile_bytes = rnn_tile_bytes(lm->dev.H, lm->dev.Vp) + 2 * align256((size_t)NN_TILE * lm->dev.H * sizeof(float));
        c.device = lm->device;
    }
    for (int s = 1; s < cfg->A; ++s)
        SCTC_CHECK_ARG(cfg->sym_word[s] >= lo && cfg->sym_word[s] <= hi, "lm_score: symbol %d maps to LM id %d outside %d..%d", s,
                       cfg->sym_word[s], lo, hi);
    c.plan = lm_score_plan(cfg->lm_kind, cfg->N, cfg->A, cfg->U_b, cfg->label_off, c.tile_bytes, terms_in_ws);
    return SCTC_OK;
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_lm_score_workspace_bytes(const sctc_lm_score_config* cfg, int32_t without_terms, size_t* bytes)
{
    SCTC_CHECK_ARG(bytes, "lm_score: null bytes");
    *bytes = 0;
    LmScoreCall c;
    SCTC_TRY(plan_lm_score(cfg, without_terms != 0, c));
    *bytes = c.plan.bytes;
    return SCTC_OK;
}

int sctc_lm_score_batch(const sctc_lm_score_config* cfg, const int32_t* labels_dev, float* terms_dev, double* sums_dev,
                        int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream)
{
    LmScoreCall c;
    SCTC_TRY(plan_lm_score(cfg, terms_dev == nullptr, c));
    if (cfg->N == 0) return SCTC_OK;
    const LmScorePlan& pl = c.plan;
    SCTC_CHECK_ARG(sums_dev && status_dev, "lm_score: null sums / status");
    SCTC_CHECK_ARG(labels_dev || pl.n_terms == 0, "lm_score: null labels");
    if (workspace_bytes < pl.bytes || !workspace_dev)
        return set_error(SCTC_ERR_WORKSPACE, "lm_score: workspace %zu bytes < %zu needed", workspace_dev ? workspace_bytes : (size_t)0,
                         pl.bytes);
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    SCTC_CHECK_ARG(dev == c.device, "lm_score: the LM lives on device %d, the current device is %d", c.device, dev);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;

    // descriptors, tiles and the symbol map: one image in the calling thread's pinned buffer (edit_distance.hip), one
    // copy into the head of the workspace
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t head = pl.off_terms;
    char* pin = (char*)stage->acquire(head);
    if (!pin) return set_error(SCTC_ERR_HIP, "lm_score: no pinned host memory for %zu bytes of descriptors", head);
    memset(pin, 0, head);
    memcpy(pin + pl.off_seqs, pl.seqs.data(), pl.seqs.size() * sizeof(LmSeq));
    if (!pl.tiles.empty()) memcpy(pin + pl.off_tiles, pl.tiles.data(), pl.tiles.size() * sizeof(LmTile));
    memcpy(pin + pl.off_sym, cfg->sym_word, (size_t)cfg->A * sizeof(int32_t));
    PinnedUploadGuard guard(s, true);
    SCTC_HIP_TRY(hipMemcpyAsync(ws, pin, head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();

    LmScoreArgs a{};
    a.seqs = (const LmSeq*)(ws + pl.off_seqs);
    a.tiles = (const LmTile*)(ws + pl.off_tiles);
    a.sym = (const int32_t*)(ws + pl.off_sym);
    a.labels = labels_dev;
    a.terms = terms_dev ? terms_dev : (float*)(ws + pl.off_terms);
    a.sums = sums_dev;
    a.status = status_dev;
    a.scratch = ws + pl.off_scratch;
    a.tile_bytes = c.tile_bytes;
    a.n_terms = pl.n_terms;
    a.n_tiles = pl.n_tiles;
    a.N = cfg->N;
    a.A = cfg->A;

    hipLaunchKernelGGL(lm_status_kernel, dim3((unsigned)((cfg->N + 3) / 4)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    if (pl.grid > 0) {
        if (cfg->lm_kind == SCTC_LM_NGRAM) {
            const sctc_lm* lm = (const sctc_lm*)cfg->lm;
            const NgramTab tab{lm->key, lm->prob, lm->bo, (uint64_t)(lm->cap - 1), lm->order, lm->bos};
            hipLaunchKernelGGL(lm_score_ngram_kernel, dim3(pl.grid), dim3(LM_SCORE_NGRAM_THREADS), 0, s, a, tab);
        } else if (cfg->lm_kind == SCTC_LM_NN) {
            hipLaunchKernelGGL(lm_score_nn_kernel, dim3(pl.grid), dim3(NN_THREADS), 0, s, a, ((const sctc_nnlm*)cfg->lm)->dev);
        } else {
            hipLaunchKernelGGL(lm_score_rnn_kernel, dim3(pl.grid), dim3(NN_THREADS), 0, s, a, ((const sctc_rnnlm*)cfg->lm)->dev);
        }
        SCTC_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(lm_sums_kernel, dim3((unsigned)((cfg->N + 255) / 256)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

// the two rank entries: `a` arrives with the word arrays set or not
static int rank_launch(bool words, int32_t B, int32_t K, const int32_t* K_b, const int32_t* U_b, double alpha, double beta,
                       const double* scores_dev, const int32_t* status_dev, const double* lm_sums_dev,
                       const double* first_scores_dev, double* rescored_dev, int32_t* order_dev, void* stream, RankArgs a)
{
    SCTC_CHECK_ARG(B >= 0, "nbest_rank: %d utterances", B);
    SCTC_CHECK_ARG(K >= 1 && K <= KMAX, "nbest_rank: %d hypotheses outside 1..%d", K, KMAX);
    if (B == 0) return SCTC_OK;
    SCTC_CHECK_ARG(K_b && U_b, "nbest_rank: null K_b / U_b");
    SCTC_CHECK_ARG(scores_dev && status_dev && rescored_dev && order_dev, "nbest_rank: null device pointer");
    for (int b = 0; b < B; ++b)
        SCTC_CHECK_ARG(K_b[b] >= 0 && K_b[b] <= K, "nbest_rank: utterance %d has %d real hypotheses, outside 0..%d", b, K_b[b], K);
    const int64_t P = (int64_t)B * K;
    for (int64_t o = 0; o < P; ++o) SCTC_CHECK_ARG(U_b[o] >= 0, "nbest_rank: pair %lld has %d labels", (long long)o, U_b[o]);
    hipStream_t s = (hipStream_t)stream;
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t bytes = (size_t)(B + P) * sizeof(int32_t);
    int32_t* pin = (int32_t*)stage->acquire(bytes);
    if (!pin) return set_error(SCTC_ERR_HIP, "nbest_rank: no pinned host memory for %zu bytes of lengths", bytes);
    memcpy(pin, K_b, (size_t)B * sizeof(int32_t));
    memcpy(pin + B, U_b, (size_t)P * sizeof(int32_t));
    void* pin_dev = nullptr;
    SCTC_HIP_TRY(hipHostGetDevicePointer(&pin_dev, pin, 0));
    a.Kb = (const int32_t*)pin_dev;
    a.U = (const int32_t*)pin_dev + B;
    a.scores = scores_dev;
    a.status = status_dev;
    a.lm = lm_sums_dev;
    a.first = first_scores_dev;
    a.out = rescored_dev;
    a.order = order_dev;
    a.alpha = alpha;
    a.beta = beta;
    a.B = B;
    a.K = K;
    PinnedUploadGuard guard(s, true);
    if (words) hipLaunchKernelGGL(nbest_rank_kernel<true>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(nbest_rank_kernel<false>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();
    return SCTC_OK;
}

int sctc_nbest_rank_batch(int32_t B, int32_t K, const int32_t* K_b, const int32_t* U_b, double alpha, double beta,
                          const double* scores_dev, const int32_t* status_dev, const double* lm_sums_dev,
                          const double* first_scores_dev, double* rescored_dev, int32_t* order_dev, void* stream)
{
    return rank_launch(false, B, K, K_b, U_b, alpha, beta, scores_dev, status_dev, lm_sums_dev, first_scores_dev,
                       rescored_dev, order_dev, stream, RankArgs{});
}

int sctc_nbest_rank_words_batch(int32_t B, int32_t K, const int32_t* K_b, const int32_t* U_b, double alpha, double beta,
                                const double* scores_dev, const int32_t* status_dev, const double* lm_sums_dev,
                                const double* first_scores_dev, const double* word_sums_dev,
                                const int32_t* word_counts_dev, const int32_t* word_status_dev, double word_alpha,
                                double word_beta, double* rescored_dev, int32_t* order_dev, void* stream)
{
    SCTC_CHECK_ARG(B <= 0 || (word_sums_dev && word_counts_dev && word_status_dev), "nbest_rank: null word-LM array");
    RankArgs a{};
    a.wsum = word_sums_dev;
    a.wcount = word_counts_dev;
    a.wstatus = word_status_dev;
    a.walpha = word_alpha;
    a.wbeta = word_beta;
    return rank_launch(true, B, K, K_b, U_b, alpha, beta, scores_dev, status_dev, lm_sums_dev, first_scores_dev,
                       rescored_dev, order_dev, stream, a);
}

}  // extern "C"
