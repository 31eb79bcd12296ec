// Word-LM scores of label sequences on the device: the fourth LM kind of the second pass.
// sctc_word_lm_score_batch turns N rows of CTC symbols into words and walks the lexicon's word LM over them, so that a
// word bigram or a word n-gram can be put on a hypothesis that did not come out of the lexicon search.
//
//   tokens   a token is a maximal run of symbols other than the space (str.split()).  Lanes read the row 64 symbols at
//            a time; a ballot of "is a space" plus the last symbol carried over from the chunk before gives the token
//            starts, and the word index of a start is the popcount below it plus the words carried.
//   words    the lane at a token start walks the prefix tree, one dependent load per symbol, on past the chunk where
//            the token does, and stops at the first miss: every step there and a word at the last node is the word's
//            id, anything else is OOV and scores as `unk`.  The ids go to the sequence's slice of the workspace.
//   terms    one lane per word: lex_bg(previous word, w) or lex_ng(history, w) of beam_policies.h, the routines and so
//            the float32 values of the lexicon search; the history is built from the up to four ids before the word
//            and <s>, across the 64-word pass.  With SCTC_WORD_LM_EOS one more term, P(</s> | history).
//   sum      float64, in word order: every lane of the wave adds the pass's terms one after the other.
//
// One wave per sequence, four to a workgroup; no atomics, no barrier between workgroups, no wait on another wave: the
// results are the same bit for bit from run to run.  A row with a symbol outside 1..A-1 never indexes a table with it.
#include <math.h>

#include <type_traits>
#include <vector>

#include "beam_lm.h"
#include "beam_policies.h"
#include "common.h"

namespace sctc {
namespace {

using namespace beam;

constexpr int WORD_LM_MAX_U = 8191;
constexpr int WORD_LM_KNOWN_FLAGS = SCTC_WORD_LM_EOS | SCTC_WORD_LM_NO_FINAL_WORD;

struct WordSeq {
    int64_t label_off;   // first label in labels_dev
    int64_t slot_off;    // first term / word id: sum over the earlier sequences of ceil(U / 2) + 1
    int32_t U;
    int32_t pad;
};

struct WordLmArgs {
    const WordSeq* seqs;     // workspace
    int32_t* ids;            // workspace: word id of every token, -1 for an OOV token
    const int32_t* labels;
    float* terms;            // or nullptr
    int32_t* word_ids;       // or nullptr
    double* sums;
    int32_t* counts;         // [N][2]
    int32_t* status;
    int32_t N, A, unk, end, eos, no_final;
};

template <bool NGRAM>
using LexTables = std::conditional_t<NGRAM, LexiconNgramArgs, LexiconArgs>;

template <bool NGRAM>
__global__ __launch_bounds__(256) void word_lm_score_kernel(WordLmArgs p, LexTables<NGRAM> lx)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= p.N) return;       // whole waves leave; there is no workgroup barrier below
    const WordSeq d = p.seqs[n];
    const int32_t* l = p.labels + d.label_off;
    int32_t* ids = p.ids + d.slot_off;
    const int U = d.U, A = p.A, space = lx.space;
    const unsigned long long below = (1ull << lane) - 1;

    // ---- tokens and their word ids ----
    bool bad = false;
    bool carry_sp = true;       // the symbol before the chunk is a space (or the row's start)
    int starts = 0, oov = 0;
    for (int base = 0; base < U; base += 64) {
        const int i = base + lane;
        const bool in = i < U;
        const int c = l[min(i, U - 1)];
        bad |= in && (c < 1 || c >= A);
        const bool sp = !in || c == space;
        const unsigned long long spm = __ballot(sp);
        const bool after_sp = lane == 0 ? carry_sp : ((spm >> (lane - 1)) & 1) != 0;
        const bool start = !sp && after_sp;
        const unsigned long long stm = __ballot(start);
        int node = -1;
        if (start) {
            node = 0;
            int j = i, cj = c;
            while (true) {
                // a symbol outside the alphabet ends the walk before it indexes the tree; the row gets status 2
                if (cj < 1 || cj >= A) {
                    node = -1;
                    break;
                }
                node = lx.child[(int64_t)node * A + cj];
                if (node < 0 || ++j >= U) break;
                cj = l[j];
                if (cj == space) break;
            }
        }
        const int at = lx.word[max(node, 0)];
        const int w = node >= 0 ? at : -1;
        oov += __popcll(__ballot(start && w < 0));
        if (start) ids[starts + __popcll(stm & below)] = w;
        starts += __popcll(stm);
        carry_sp = (spm >> 63) != 0;
    }
    // Every lane reads below, from global memory, ids that other lanes of this wave stored above.  What makes that
    // safe is the workgroup-scope release / acquire pair around the wave barrier: on gfx950 a wave's vector memory
    // operations go in order through the CU's one L1 (the workgroup is not split over CUs), so the fences cost a wait and
    // no cache maintenance -- but without them, or with the ids read through a path the compiler may turn into scalar
    // loads (another cache), a lane could see the workspace's old contents.  Keep both fences and keep `ids` a plain
    // per-lane vector load.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // ---- the words that count ----
    int last = space;
    if (U > 0) last = l[U - 1];
    const bool dropped = p.no_final != 0 && last != space;      // the last token has no space after it
    const int W = starts - (dropped ? 1 : 0);
    if (dropped && ids[starts - 1] < 0) oov -= 1;
    const int st = __any(bad) ? 2 : (p.unk < 0 && oov > 0 ? 3 : 0);

    // ---- terms and their sum ----
    double sum = st == 0 ? 0.0 : -INFINITY;
    const int n_terms = st == 0 ? W + (p.eos ? 1 : 0) : 0;
    // The reads of ids[] below use clamped indices and a select: with no words (the </s> term alone) and for the history
    // before the first word they touch ids[0], which may hold whatever the workspace held.  The slot is inside the
    // sequence's slice (every sequence owns at least one), and the value read is discarded by the select.
    for (int k0 = 0; k0 < n_terms; k0 += 64) {
        const int k = min(k0 + lane, n_terms - 1);
        const int own = ids[max(min(k, W - 1), 0)];
        const int w = k < W ? (own < 0 ? p.unk : own) : p.end;
        int32_t h[NG_HIST];
#pragma unroll
        for (int j = 0; j < NG_HIST; ++j) {
            const int idx = k - 1 - j;
            const int v = ids[max(idx, 0)];
            h[j] = idx >= 0 ? (v < 0 ? p.unk : v) : (idx == -1 ? lx.start : -1);
        }
        float term;
        if constexpr (NGRAM) {
#pragma unroll
            for (int j = 0; j < NG_HIST; ++j) h[j] = j < lx.order - 1 ? h[j] : -1;
            term = lex_ng(lx, h, w);
        } else {
            term = lex_bg(lx, h[0], w);
        }
        if (k0 + lane < n_terms) {
            if (p.terms) p.terms[d.slot_off + k] = term;
            if (p.word_ids) p.word_ids[d.slot_off + k] = w;
        }
        const int cnt = min(64, n_terms - k0);
        for (int j = 0; j < cnt; ++j) sum += (double)__shfl(term, j);
    }
    if (lane == 0) {
        p.sums[n] = sum;
        p.counts[2 * n] = st == 2 ? 0 : W;
        p.counts[2 * n + 1] = st == 2 ? 0 : oov;
        p.status[n] = st;
    }
}

struct WordLmPlan {
    std::vector<WordSeq> seqs;
    int64_t n_slots = 0;
    size_t off_ids = 0, bytes = 0;
};

// the output and label pointers of the batch entry; the workspace query has none
struct WordLmPointers {
    const void* labels;
    const void* sums;
    const void* counts;
    const void* status;
};

// the checks that need no device, then the descriptors and the two slices of the workspace.  Everything that can be
// told without the handle is told before it is read; of the handle's own checks the word range comes before the
// alphabet.
int plan_word_lm(const sctc_word_lm_score_config* cfg, const WordLmPointers* io, WordLmPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "word_lm_score: null config");
    SCTC_CHECK_ARG(cfg->N >= 0, "word_lm_score: %d sequences", cfg->N);
    SCTC_CHECK_ARG(cfg->A >= 1 && cfg->A <= AMAX, "word_lm_score: alphabet of %d symbols outside 1..%d", cfg->A, AMAX);
    SCTC_CHECK_ARG((cfg->flags & ~WORD_LM_KNOWN_FLAGS) == 0, "word_lm_score: unknown flags 0x%x", cfg->flags);
    SCTC_CHECK_ARG(cfg->lexicon, "word_lm_score: null lexicon");
    SCTC_CHECK_ARG(cfg->unk >= -1 && cfg->end >= -1, "word_lm_score: <UNK> id %d / </s> id %d below -1", cfg->unk, cfg->end);
    SCTC_CHECK_ARG(!(cfg->flags & SCTC_WORD_LM_EOS) || cfg->end >= 0, "word_lm_score: the </s> term asked without a </s> id");
    SCTC_CHECK_ARG(cfg->N == 0 || (cfg->U_b && cfg->label_off), "word_lm_score: null length / offset array");
    for (int n = 0; n < cfg->N; ++n) {
        SCTC_CHECK_ARG(cfg->U_b[n] >= 0 && cfg->U_b[n] <= WORD_LM_MAX_U, "word_lm_score: sequence %d has %d labels, outside 0..%d",
                       n, cfg->U_b[n], WORD_LM_MAX_U);
        SCTC_CHECK_ARG(cfg->label_off[n] >= 0, "word_lm_score: sequence %d has a negative offset", n);
    }
    if (io && cfg->N > 0) {
        SCTC_CHECK_ARG(io->sums && io->counts && io->status, "word_lm_score: null sums / counts / status");
        bool any = false;
        for (int n = 0; n < cfg->N; ++n) any |= cfg->U_b[n] > 0;
        SCTC_CHECK_ARG(io->labels || !any, "word_lm_score: null labels");
    }
    // what follows reads the handle
    const sctc_lexicon* h = cfg->lexicon;
    SCTC_CHECK_ARG(cfg->unk < h->n_words && cfg->end < h->n_words, "word_lm_score: <UNK> id %d / </s> id %d outside %lld words",
                   cfg->unk, cfg->end, (long long)h->n_words);
    SCTC_CHECK_ARG(cfg->A == h->A, "word_lm_score: the lexicon was built for %d symbols, the config has %d", h->A, cfg->A);
    pl.seqs.resize(cfg->N);
    int64_t slot = 0;
    for (int n = 0; n < cfg->N; ++n) {
        pl.seqs[n] = WordSeq{cfg->label_off[n], slot, cfg->U_b[n], 0};
        slot += (cfg->U_b[n] + 1) / 2 + 1;
    }
    pl.n_slots = slot;
    pl.off_ids = align256((size_t)cfg->N * sizeof(WordSeq));
    pl.bytes = pl.off_ids + align256((size_t)slot * sizeof(int32_t));
    return SCTC_OK;
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_word_lm_score_workspace_bytes(const sctc_word_lm_score_config* cfg, size_t* bytes)
{
    SCTC_CHECK_ARG(bytes, "word_lm_score: null bytes");
    *bytes = 0;
    WordLmPlan pl;
    SCTC_TRY(plan_word_lm(cfg, nullptr, pl));
    *bytes = pl.bytes;
    return SCTC_OK;
}

int sctc_word_lm_score_batch(const sctc_word_lm_score_config* cfg, const int32_t* labels_dev, float* terms_dev,
                             int32_t* word_ids_dev, double* sums_dev, int32_t* counts_dev, int32_t* status_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream)
{
    WordLmPlan pl;
    const WordLmPointers io{labels_dev, sums_dev, counts_dev, status_dev};
    SCTC_TRY(plan_word_lm(cfg, &io, pl));
    if (cfg->N == 0) return SCTC_OK;
    if (workspace_bytes < pl.bytes || !workspace_dev)
        return set_error(SCTC_ERR_WORKSPACE, "word_lm_score: workspace %zu bytes < %zu needed",
                         workspace_dev ? workspace_bytes : (size_t)0, pl.bytes);
    const sctc_lexicon* h = cfg->lexicon;
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    SCTC_CHECK_ARG(dev == h->device, "word_lm_score: the lexicon lives on device %d, the current device is %d", h->device, dev);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;

    // the descriptors: one image in the calling thread's pinned buffer, one copy into the head of the workspace
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t head = (size_t)cfg->N * sizeof(WordSeq);
    char* pin = (char*)stage->acquire(head);
    if (!pin) return set_error(SCTC_ERR_HIP, "word_lm_score: no pinned host memory for %zu bytes of descriptors", head);
    memcpy(pin, pl.seqs.data(), head);
    PinnedUploadGuard guard(s, true);
    SCTC_HIP_TRY(hipMemcpyAsync(ws, pin, head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();

    WordLmArgs a{};
    a.seqs = (const WordSeq*)ws;
    a.ids = (int32_t*)(ws + pl.off_ids);
    a.labels = labels_dev;
    a.terms = terms_dev;
    a.word_ids = word_ids_dev;
    a.sums = sums_dev;
    a.counts = counts_dev;
    a.status = status_dev;
    a.N = cfg->N;
    a.A = cfg->A;
    a.unk = cfg->unk;
    a.end = cfg->end;
    a.eos = (cfg->flags & SCTC_WORD_LM_EOS) != 0;
    a.no_final = (cfg->flags & SCTC_WORD_LM_NO_FINAL_WORD) != 0;
    const dim3 grid((unsigned)((cfg->N + 3) / 4));
    if (h->order) {
        LexiconNgramArgs ng{};
        ng.child = h->child;
        ng.word = h->word;
        ng.ug = h->ug;
        ng.bo = h->bo;
        ng.key = h->bg_key;
        ng.val = h->bg_val;
        ng.nbo = h->ng_bo;
        ng.id = h->ng_id;
        ng.mask = (uint64_t)(h->bg_cap - 1);
        ng.start = h->start;
        ng.space = h->space;
        ng.order = h->order;
        hipLaunchKernelGGL(word_lm_score_kernel<true>, grid, dim3(256), 0, s, a, ng);
    } else {
        LexiconArgs lx{};
        lx.child = h->child;
        lx.word = h->word;
        lx.ug = h->ug;
        lx.bo = h->bo;
        lx.key = h->bg_key;
        lx.val = h->bg_val;
        lx.mask = (uint64_t)(h->bg_cap - 1);
        lx.start = h->start;
        lx.space = h->space;
        hipLaunchKernelGGL(word_lm_score_kernel<false>, grid, dim3(256), 0, s, a, lx);
    }
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
