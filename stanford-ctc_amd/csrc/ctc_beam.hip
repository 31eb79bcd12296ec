// CTC prefix beam search with a character n-gram LM: the reference's BeamLMDecoder.decode
// (ctc_fast/new_decoder/decoder.pyx:136-193) for a batch of utterances, one workgroup per
// utterance, every frame of the search inside one launch.  DESIGN.md §4.5 has the semantics
// and the design points; in short, per frame:
//   1. cells: beam entry j (rank order) and symbol c form cell j*A + c -- c == 0 is the
//      prefix itself (blank and repeat terms, plus its parent's extension when the parent is
//      in the beam), c >= 1 the extension P+c (LM term, plus the "Hold" masses of P+c among
//      the previous frame's candidates); an extension that IS a beam entry is disabled (its
//      mass arrives through that entry's own cell), so every prefix is counted once;
//   2. top-`beam` select: radix select over order-preserving 64-bit keys of the float64
//      sort key, ties by ascending cell index; then ranks by counting;
//   3. the new beam: float32 masses, 64-bit prefix hashes, LM context, a back-pointer per
//      entry and frame (the hypotheses are read back through them at the end);
//   4. LM rows (log10 P(c | <s> + P) for all c) for the entries that are new; an entry that
//      carried over keeps its row.
//
// The same body, instantiated a second time (LEX), is the lexicon-constrained word-bigram search
// (the reference's ctc_fast/decoder/bg_decoder.pyx:18-95): every beam entry also
// carries its prefix-tree node, the previous word, the word count and the cached bigram term of
// its space extension; an extension the tree forbids is no candidate, the LM term is the word
// bigram at a space, and the length bonus counts words.
//
// A third instantiation (NN) is the character search with a neural LM as the provider of the rows
// (the lexicon-free path of the reference's ctc_fast/decoder/clm_decoder2.pyx): every
// beam entry carries the window of the last K LM ids of <null>.. <s> + P, copied from its parent and
// shifted on extension, and step 4 evaluates the rows of the new entries in tiles of 32 through
// nnlm_tile (nnlm_dev.h), the routine sctc_nnlm_rows runs.
//
// A fourth instantiation (RNN) takes the rows from a recurrent neural LM (the `rnn` model type of
// clm_decoder2.pyx): every beam entry carries the LM's hidden state of its prefix,
// copied from its parent when carried over; step 4 makes one recurrent step per new entry, from the
// parent's state and the new symbol, in tiles of 32 through rnnlm_tile (rnnlm_dev.h), the routine
// sctc_rnnlm_step runs.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "common.h"
#include "nnlm_dev.h"
#include "rnnlm_dev.h"

struct sctc_lm {
    uint64_t* key = nullptr;   // device [cap]; prob / backoff follow in the same allocation
    float* prob = nullptr;
    float* bo = nullptr;
    int64_t cap = 0;
    int32_t order = 0;
    int32_t bos = 0;
    int device = -1;
};

// The device lexicon of the word-bigram search: the flattened prefix tree (dense child table,
// word id per node), the unigram arrays and an open-addressing table of the listed bigrams.
struct sctc_lexicon {
    char* mem = nullptr;        // one allocation; the arrays below point into it
    int32_t* child = nullptr;   // [nodes * A]: child node of (node, symbol), -1 for none
    int32_t* word = nullptr;    // [nodes]: word id of the word ending here, -1 for none
    float* ug = nullptr;        // [n_words] unigram value
    float* bo = nullptr;        // [n_words] unigram back-off
    uint64_t* bg_key = nullptr; // [bg_cap] (w1 << 32) | w2, all ones = empty
    float* bg_val = nullptr;    // [bg_cap]
    int64_t nodes = 0, n_words = 0, bg_cap = 0;
    size_t bytes = 0;
    int32_t A = 0, start = 0;
    int device = -1;
};

namespace sctc {
namespace {

constexpr int NT = 256;       // threads per workgroup
constexpr int KMAX = 256;     // beam limit
constexpr int AMAX = 256;     // alphabet limit
constexpr int HT = 512;       // slots of a beam hash table (load <= 1/2)
constexpr uint64_t H_EMPTY_PREFIX = 0x6A09E667F3BCC909ull;

struct UttDesc {
    int64_t frame_off;   // first row of the utterance in probs
    int64_t ws_off;      // byte offset of its workspace slice
    int64_t id_off;      // first hypothesis element: ids[nbest * id_off + n * T + i]
    int32_t T;
    int32_t pad;
};

struct BeamArgs {
    const void* probs;
    int64_t ld;
    int32_t f64;
    int32_t A, K, nbest;
    double alpha, beta;
    const UttDesc* utt;
    const int32_t* sym_word;   // device [A]
    char* ws;
    const uint64_t* lm_key;    // nullptr: no LM term
    const float* lm_prob;
    const float* lm_bo;
    uint64_t lm_mask;
    int32_t lm_order, lm_bos;
    int32_t* ids;
    int32_t* lens;
    double* scores;
    // the lexicon search only
    const int32_t* lx_child;
    const int32_t* lx_word;
    const float* lx_ug;
    const float* lx_bo;
    const uint64_t* lx_key;
    const float* lx_val;
    uint64_t lx_mask;
    int32_t lx_start, space;
};

constexpr uint64_t BG_EMPTY = ~0ull;

// the neural LM search only: a kernel argument of its own, BeamArgs stays as the other two read it
struct NNArgs {
    NNLMDev m;
};
struct NoNNArgs {
};
// the recurrent LM search only
struct RNNArgs {
    RNNLMDev m;
    int32_t state_copies;   // 1; SCTC_RNNBEAM_STATE_COPIES = 2..4 repeats the copy of the carried states, which
                            // changes no result: the time it adds is what the copy costs (tools/decode_rnn_bench.py)
};
constexpr int WIN = NN_MAX_CONTEXT;   // bytes of a beam entry's context window (one LM id per byte)

// workspace slices are 256-byte aligned on both sides of the launch
__host__ __device__ inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ __device__ inline uint64_t mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// hash of the prefix P+c from the hash of P: a bijection of h for fixed c, and of c for fixed h
__device__ inline uint64_t hstep(uint64_t h, int c) { return mix64(h ^ ((uint64_t)(c + 1) * 0xD6E8FEB86659FD93ull)); }

// order-preserving map double -> uint64 (larger double, larger key); 0 is never produced
__device__ inline uint64_t okey(double d)
{
    const uint64_t u = (uint64_t)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double okey_inv(uint64_t k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// max-shifted log(exp a + exp b (+ exp c)); -inf for all -inf (decoder.pyx:32-37 without the shift)
__device__ inline double lse2(double a, double b)
{
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m));
}
__device__ inline double lse3(double a, double b, double c)
{
    const double m = fmax(fmax(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

__device__ inline uint64_t bytes_mask(int m) { return m >= 8 ? ~0ull : ((1ull << (8 * m)) - 1); }

__device__ inline bool lm_find(const BeamArgs& p, uint64_t key, float& pr, float& bo)
{
    uint64_t s = mix64(key) & p.lm_mask;
    while (true) {
        const uint64_t k = p.lm_key[s];
        if (k == key) {
            pr = p.lm_prob[s];
            bo = p.lm_bo[s];
            return true;
        }
        if (k == 0) return false;
        s = (s + 1) & p.lm_mask;
    }
}

// log10 P(w | ctx): ctx = the last `ctxlen` word ids (newest in the low byte, <s> included);
// longest n-gram first found by growing the context, then the back-offs of the longer contexts
// in increasing length, float32 additions in kenlm's order (arpa_lm.ArpaLM.score_ids)
__device__ float lm_score(const BeamArgs& p, uint64_t ctx, int ctxlen, uint32_t w)
{
    float pr = -100.0f, bo = 0.0f;
    lm_find(p, w, pr, bo);              // every word id the host maps to is a unigram
    float best = pr;
    int n = 1;
    for (int m = 1; m <= ctxlen; ++m) {
        if (!lm_find(p, ((ctx & bytes_mask(m)) << 8) | w, pr, bo)) break;
        best = pr;
        n = m + 1;
    }
    for (int m = n; m <= ctxlen; ++m) {
        if (!lm_find(p, ctx & bytes_mask(m), pr, bo)) break;
        best = best + bo;
    }
    return best;
}

// bg_prob(w1, w2) of fastdecode/lm.cpp:119-127: the listed bigram, or -- when there is none or it
// is exactly 0 -- the float32 sum back-off(w1) + unigram(w2)
__device__ inline float lex_bg(const BeamArgs& p, int w1, int w2)
{
    const uint64_t key = ((uint64_t)(uint32_t)w1 << 32) | (uint32_t)w2;
    uint64_t s = mix64(key) & p.lx_mask;
    float v = 0.0f;
    while (true) {
        const uint64_t k = p.lx_key[s];
        if (k == key) {
            v = p.lx_val[s];
            break;
        }
        if (k == BG_EMPTY) break;
        s = (s + 1) & p.lx_mask;
    }
    if (v == 0.0f) v = p.lx_bo[w1] + p.lx_ug[w2];
    return v;
}

// per beam entry of the lexicon search; a function of the prefix alone
template <bool LEX>
struct LexState {
    int32_t node[KMAX];   // prefix-tree node the unfinished word has reached (0 = root)
    int32_t pw[KMAX];     // id of the last finished word (<s> at the start)
    int32_t nw[KMAX];     // finished words
    int32_t wd[KMAX];     // word id of `node`, -1: a space cannot follow
    float bg[KMAX];       // bg_prob(pw, wd): the LM value of the space extension, 0 without one
};
template <>
struct LexState<false> {
};

struct Beam {
    uint64_t h[KMAX];     // prefix hash
    uint64_t ph[KMAX];    // hash of the prefix without its last symbol
    uint64_t ctx[KMAX];   // LM context: last (order-1) word ids of <s> + P
    double key[KMAX];     // float64 sort key of the cell it came from
    float pnb[KMAX], pb[KMAX];
    int32_t last[KMAX];   // last symbol, -1 for the empty prefix
    int32_t len[KMAX];
    int32_t prev[KMAX];   // rank in the previous frame's beam when carried over, else -1
};

struct HTab {
    uint64_t key[HT];
    int32_t idx[HT];
};

__device__ inline int htab_find(const HTab& t, uint64_t h)
{
    int s = (int)(h & (HT - 1));
    while (true) {
        const int i = t.idx[s];
        if (i < 0) return -1;
        if (t.key[s] == h) return i;
        s = (s + 1) & (HT - 1);
    }
}

__device__ inline void htab_insert(HTab& t, uint64_t h, int i)
{
    int s = (int)(h & (HT - 1));
    while (atomicCAS(&t.idx[s], -1, i) != -1) s = (s + 1) & (HT - 1);
    t.key[s] = h;
}

// exclusive prefix sum over the workgroup (NT threads, wave64); *total = sum of all
__device__ int block_excl_scan(int v, int* scratch, int* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) scratch[wv] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < NT / 64; ++i) {
        const int s = scratch[i];
        if (i < wv) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

__device__ inline double load_prob(const BeamArgs& p, int64_t row, int c)
{
    return p.f64 ? ((const double*)p.probs)[row * p.ld + c] : (double)((const float*)p.probs)[row * p.ld + c];
}

// NN: a neural LM supplies the rows -- the window model, or with RNN the recurrent one
template <bool LEX, bool NN, bool RNN, typename NNA>
__device__ __forceinline__ void beam_search(const BeamArgs& p, const NNA& nn)
{
    static_assert(NN || !RNN, "the recurrent LM is a neural LM");
    __shared__ Beam bm[2];
    __shared__ LexState<LEX> lx[2];
    __shared__ HTab tab[2];
    __shared__ double y[AMAX];
    __shared__ int32_t par[KMAX];
    __shared__ uint64_t sel_key[KMAX];
    __shared__ int32_t sel_idx[KMAX];
    __shared__ int32_t hist[256];
    __shared__ int32_t scan_scratch[NT / 64];
    __shared__ int32_t s_bin, s_above, s_cnt, s_count;

    const int tid = threadIdx.x;
    const UttDesc u = p.utt[blockIdx.x];
    const int A = p.A, K = p.K, T = u.T;
    const int64_t M = (int64_t)K * A;
    const bool has_lm = NN || (!LEX && p.lm_key != nullptr);
    const int ctx_max = has_lm ? p.lm_order - 1 : 0;
    const uint64_t ctx_mask = bytes_mask(ctx_max);

    char* w = p.ws + u.ws_off;
    float2* cand[2] = {(float2*)w, (float2*)w + M};
    w += al256(2 * M * sizeof(float2));
    uint64_t* ckey = (uint64_t*)w;
    w += al256(M * sizeof(uint64_t));
    float* rows[2] = {(float*)w, (float*)w + M};
    if (has_lm) w += al256(2 * M * sizeof(float));
    // NN: the context windows of both beams, then the scratch of one LM tile
    uint8_t* win[2] = {nullptr, nullptr};
    float* nn_act = nullptr;
    float* nn_rows = nullptr;
    int32_t* nn_ids = nullptr;
    // RNN: the hidden states of both beams, [2][K][H], then the scratch of one LM tile
    float* st[2] = {nullptr, nullptr};
    int32_t* nn_slot = nullptr;
    if constexpr (RNN) {
        const int H = nn.m.H;
        st[0] = (float*)w;
        st[1] = st[0] + (size_t)K * H;
        w += al256((size_t)2 * K * H * sizeof(float));
        nn_act = (float*)w;
        nn_rows = (float*)(w + nn_act_bytes(H));
        nn_slot = (int32_t*)(w + nn_act_bytes(H) + nn_row_bytes(nn.m.Vp));
        w += rnn_tile_bytes(H, nn.m.Vp);
    } else if constexpr (NN) {
        win[0] = (uint8_t*)w;
        win[1] = win[0] + (size_t)K * WIN;
        w += al256((size_t)2 * K * WIN);
        nn_act = (float*)w;
        nn_rows = (float*)(w + nn_act_bytes(nn.m.hmax));
        nn_ids = (int32_t*)(w + nn_act_bytes(nn.m.hmax) + nn_row_bytes(nn.m.Vp));
        w += nn_tile_bytes(nn.m.hmax, nn.m.Vp, nn.m.K);
    }
    int32_t* rec = (int32_t*)w;

    for (int s = tid; s < HT; s += NT) {
        tab[0].idx[s] = -1;
        tab[1].idx[s] = -1;
    }
    if (tid == 0) {
        bm[0].h[0] = H_EMPTY_PREFIX;
        bm[0].ph[0] = 0;
        bm[0].ctx[0] = has_lm ? ((uint64_t)p.lm_bos & ctx_mask) : 0;
        bm[0].key[0] = 0.0;
        bm[0].pnb[0] = -INFINITY;
        bm[0].pb[0] = 0.0f;
        bm[0].last[0] = -1;
        bm[0].len[0] = 0;
        bm[0].prev[0] = -1;
        if constexpr (LEX) {
            lx[0].node[0] = 0;
            lx[0].pw[0] = p.lx_start;
            lx[0].nw[0] = 0;
            lx[0].wd[0] = p.lx_word[0];
            lx[0].bg[0] = 0.0f;
        }
    }
    __syncthreads();
    if (tid == 0) htab_insert(tab[0], H_EMPTY_PREFIX, 0);
    if constexpr (RNN) {
        // the empty prefix: <s> into the zero state
        if (tid == 0) {
            nn_slot[0] = nn.m.bos;
            nn_slot[NN_TILE] = 0;
            nn_slot[2 * NN_TILE] = 0;
        }
        __syncthreads();
        rnnlm_tile(nn.m, nn_slot, 1, nullptr, st[0], nn_act, nn_rows);
        for (int c = tid; c < A; c += NT) rows[0][c] = c == 0 ? 0.0f : nn_rows[p.sym_word[c]];
    } else if constexpr (NN) {
        // the empty prefix: <null> .. <null> <s>
        const int CK = nn.m.K;
        for (int s = tid; s < CK; s += NT) {
            const int id = s == CK - 1 ? nn.m.bos : nn.m.null_id;
            win[0][s] = (uint8_t)id;
            nn_ids[s] = id;
        }
        __syncthreads();
        nnlm_tile(nn.m, nn_ids, 1, nn_act, nn_rows);
        for (int c = tid; c < A; c += NT) rows[0][c] = c == 0 ? 0.0f : nn_rows[p.sym_word[c]];
    } else {
        if (has_lm)
            for (int c = tid; c < A; c += NT)
                rows[0][c] = c == 0 ? 0.0f : lm_score(p, bm[0].ctx[0], ctx_max < 1 ? ctx_max : 1, (uint32_t)p.sym_word[c]);
    }
    __syncthreads();

    int n = 1, cb = 0, tc = 0, rb = 0;
    for (int t = 0; t < T; ++t) {
        const Beam& B = bm[cb];
        Beam& NB = bm[cb ^ 1];
        const LexState<LEX>& X = lx[cb];
        LexState<LEX>& NX = lx[cb ^ 1];
        const HTab& cur = tab[tc];
        const HTab& old = tab[tc ^ 1];
        const int cw = t & 1, cr = cw ^ 1;
        const int64_t row = u.frame_off + t;
        for (int c = tid; c < A; c += NT) y[c] = load_prob(p, row, c);
        for (int j = tid; j < n; j += NT) par[j] = B.len[j] > 0 ? htab_find(cur, B.ph[j]) : -1;
        __syncthreads();

        // ---- 1. cells ----------------------------------------------------------------------
        const int Mn = n * A;
        const double y0 = y[0];
        for (int idx = tid; idx < Mn; idx += NT) {
            const int j = idx / A, c = idx - j * A;
            const double v0 = (double)B.pnb[j], v1 = (double)B.pb[j];
            const int l = B.last[j];
            double nb, bb;
            int klen;
            if (c == 0) {
                nb = -INFINITY;
                if (B.len[j] > 0) {
                    const double t0 = v0 + y[l];
                    const int pj = par[j];
                    if (pj >= 0) {
                        double lmp;
                        if constexpr (LEX) lmp = l == p.space ? p.alpha * (double)X.bg[pj] : 0.0;
                        else lmp = has_lm ? p.alpha * (double)rows[rb][pj * A + l] : 0.0;
                        const double e1 = (double)B.pb[pj] + y[l] + lmp;
                        const double e0 = B.last[pj] != l ? (double)B.pnb[pj] + y[l] + lmp : -INFINITY;
                        nb = lse3(t0, e0, e1);
                    } else {
                        nb = t0;
                    }
                }
                bb = lse2(v0 + y0, v1 + y0);
                klen = B.len[j];
                if constexpr (LEX) klen = X.nw[j];
            } else {
                if constexpr (LEX) {
                    // a space only after a whole word, a letter only along the tree: anything
                    // else is no candidate (bg_decoder.pyx:48-61)
                    const bool ok = c == p.space ? X.wd[j] >= 0 : p.lx_child[(int64_t)X.node[j] * A + c] >= 0;
                    if (!ok) {
                        ckey[idx] = 0;
                        cand[cw][idx] = make_float2(-INFINITY, -INFINITY);
                        continue;
                    }
                }
                const uint64_t H = hstep(B.h[j], c);
                if (htab_find(cur, H) >= 0) {          // P+c is a beam entry: counted there
                    ckey[idx] = 0;
                    cand[cw][idx] = make_float2(-INFINITY, -INFINITY);
                    continue;
                }
                double lmw;
                if constexpr (LEX) lmw = c == p.space ? p.alpha * (double)X.bg[j] : 0.0;
                else lmw = has_lm ? p.alpha * (double)rows[rb][idx] : 0.0;
                const double e1 = v1 + y[c] + lmw;
                const double e0 = c != l ? v0 + y[c] + lmw : -INFINITY;
                float2 hv = make_float2(-INFINITY, -INFINITY);
                const int q = htab_find(old, H);
                if (q >= 0) hv = cand[cr][(int64_t)q * A];
                else if (B.prev[j] >= 0) hv = cand[cr][(int64_t)B.prev[j] * A + c];
                nb = lse3(e0, e1, (double)hv.x + y[c]);
                bb = lse2((double)hv.x + y0, (double)hv.y + y0);
                klen = B.len[j] + 1;
                if constexpr (LEX) klen = X.nw[j] + (c == p.space);
            }
            const double key = lse2(nb, bb) + p.beta * (double)klen;
            ckey[idx] = okey(key);
            cand[cw][idx] = make_float2((float)nb, (float)bb);
        }
        __syncthreads();

        // ---- 2. select the K best cells: radix select on the keys ------------------------
        uint64_t prefix = 0;
        int need = K, level = 64;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int idx = tid; idx < Mn; idx += NT) {
                const uint64_t k = ckey[idx];
                if (k == 0) continue;
                if (shift < 56 && (k >> (shift + 8)) != (prefix >> (shift + 8))) continue;
                atomicAdd(&hist[(k >> shift) & 255], 1);
            }
            __syncthreads();
            const int v = hist[255 - tid];
            int total;
            const int above = block_excl_scan(v, scan_scratch, &total);
            if (shift == 56 && total <= need) break;     // every eligible cell is kept
            if (above < need && above + v >= need) {
                s_bin = 255 - tid;
                s_above = above;
                s_cnt = v;
            }
            __syncthreads();
            prefix |= (uint64_t)s_bin << shift;
            need -= s_above;
            level = shift;
            const bool done = s_cnt == need;
            __syncthreads();
            if (done) break;
        }
        if (tid == 0) s_count = 0;
        __syncthreads();
        for (int idx = tid; idx < Mn; idx += NT) {
            const uint64_t k = ckey[idx];
            if (k == 0) continue;
            if (level == 64 || (k >> level) > (prefix >> level)) {
                const int pos = atomicAdd(&s_count, 1);
                sel_key[pos] = k;
                sel_idx[pos] = idx;
            }
        }
        __syncthreads();
        int nsel = s_count;
        if (level < 64) {
            // ties with the threshold: the first `need` in cell order
            const int chunk = (Mn + NT - 1) / NT;
            const int beg = tid * chunk, end = min(Mn, beg + chunk);
            int mine = 0;
            for (int idx = beg; idx < end; ++idx) {
                const uint64_t k = ckey[idx];
                mine += (k != 0 && (k >> level) == (prefix >> level));
            }
            int total;
            int rank = block_excl_scan(mine, scan_scratch, &total);
            for (int idx = beg; idx < end && rank < need; ++idx) {
                const uint64_t k = ckey[idx];
                if (k != 0 && (k >> level) == (prefix >> level)) {
                    sel_key[nsel + rank] = k;
                    sel_idx[nsel + rank] = idx;
                    ++rank;
                }
            }
            nsel += need;
            __syncthreads();
        }

        // ---- 3. ranks by counting, the new beam --------------------------------------------
        if (tid < nsel) {
            const uint64_t k = sel_key[tid];
            const int ix = sel_idx[tid];
            int r = 0;
            for (int i = 0; i < nsel; ++i) {
                const uint64_t ki = sel_key[i];
                r += (ki > k) || (ki == k && sel_idx[i] < ix);
            }
            const int j = ix / A, c = ix - j * A;
            const float2 cv = cand[cw][ix];
            NB.pnb[r] = cv.x;
            NB.pb[r] = cv.y;
            NB.key[r] = okey_inv(k);
            if (c == 0) {
                NB.h[r] = B.h[j];
                NB.ph[r] = B.ph[j];
                NB.ctx[r] = B.ctx[j];
                NB.last[r] = B.last[j];
                NB.len[r] = B.len[j];
                NB.prev[r] = j;
                if constexpr (LEX) {
                    NX.node[r] = X.node[j];
                    NX.pw[r] = X.pw[j];
                    NX.nw[r] = X.nw[j];
                    NX.wd[r] = X.wd[j];
                    NX.bg[r] = X.bg[j];
                }
                if constexpr (NN && !RNN) {
                    const uint4* src = (const uint4*)(win[cb] + (size_t)j * WIN);
                    uint4* dst = (uint4*)(win[cb ^ 1] + (size_t)r * WIN);
                    dst[0] = src[0];
                    dst[1] = src[1];
                }
            } else {
                NB.h[r] = hstep(B.h[j], c);
                NB.ph[r] = B.h[j];
                NB.ctx[r] = has_lm ? (((B.ctx[j] << 8) | (uint64_t)p.sym_word[c]) & ctx_mask) : 0;
                NB.last[r] = c;
                NB.len[r] = B.len[j] + 1;
                NB.prev[r] = -1;
                if constexpr (LEX) {
                    const bool sp = c == p.space;
                    const int nd = sp ? 0 : p.lx_child[(int64_t)X.node[j] * A + c];
                    const int pw = sp ? X.wd[j] : X.pw[j];
                    const int wd = p.lx_word[nd];
                    NX.node[r] = nd;
                    NX.pw[r] = pw;
                    NX.nw[r] = X.nw[j] + sp;
                    NX.wd[r] = wd;
                    NX.bg[r] = wd >= 0 ? lex_bg(p, pw, wd) : 0.0f;
                }
                if constexpr (NN && !RNN) {
                    // the parent's window, one slot older, and the new symbol's LM id
                    const uint8_t* src = win[cb] + (size_t)j * WIN;
                    uint8_t* dst = win[cb ^ 1] + (size_t)r * WIN;
                    const int CK = nn.m.K;
                    for (int s = 0; s + 1 < CK; ++s) dst[s] = src[s + 1];
                    dst[CK - 1] = (uint8_t)p.sym_word[c];
                }
            }
            rec[(int64_t)t * K + r] = (j << 16) | c;
        }
        // the previous beam's table is no longer needed: it becomes the new beam's
        HTab& nt = tab[tc ^ 1];
        for (int s = tid; s < HT; s += NT) nt.idx[s] = -1;
        __syncthreads();
        if (tid < nsel) htab_insert(nt, NB.h[tid], tid);

        // ---- 4. LM rows: carried entries keep theirs, new ones query the LM ----------------
        if constexpr (NN) {
            for (int it = tid; it < nsel * A; it += NT) {
                const int r = it / A;
                const int src = NB.prev[r];
                if (src >= 0) rows[rb ^ 1][it] = rows[rb][src * A + (it - r * A)];
            }
            if constexpr (RNN) {
                // a carried entry keeps its state: a copy into the new beam's buffer
                const int Hq = nn.m.H >> 2;
                const float4* so = (const float4*)st[cb];
                float4* sn = (float4*)st[cb ^ 1];
                for (int pass = 0; pass < nn.state_copies; ++pass)
                    for (int it = tid; it < nsel * Hq; it += NT) {
                        const int r = it / Hq;
                        const int src = NB.prev[r];
                        if (src >= 0) sn[it] = so[(size_t)src * Hq + (it - r * Hq)];
                    }
            }
            // the new entries in rank order, 32 to a tile (sel_idx is free until the next select)
            const int fresh = tid < nsel && NB.prev[tid] < 0;
            int n_new;
            const int pos = block_excl_scan(fresh, scan_scratch, &n_new);
            if (fresh) sel_idx[pos] = tid;
            __syncthreads();
            const int Vp = nn.m.Vp;
            int CK = 0;
            const uint8_t* wn = nullptr;
            if constexpr (!RNN) {
                CK = nn.m.K;
                wn = win[cb ^ 1];
            }
            for (int t0 = 0; t0 < n_new; t0 += NN_TILE) {
                const int cnt = min(NN_TILE, n_new - t0);
                if constexpr (RNN) {
                    // the parent j and the symbol c as step 3 recorded them: the parent's state is in
                    // the old beam's buffer, the entry's goes to the new one
                    if (tid < cnt) {
                        const int r = sel_idx[t0 + tid];
                        const int ev = rec[(int64_t)t * K + r];
                        nn_slot[tid] = p.sym_word[ev & 0xFFFF];
                        nn_slot[NN_TILE + tid] = ev >> 16;
                        nn_slot[2 * NN_TILE + tid] = r;
                    }
                    __syncthreads();
                    rnnlm_tile(nn.m, nn_slot, cnt, st[cb], st[cb ^ 1], nn_act, nn_rows);
                } else {
                    for (int i = tid; i < cnt * CK; i += NT) {
                        const int e = i / CK, s = i - e * CK;
                        nn_ids[i] = wn[(size_t)sel_idx[t0 + e] * WIN + s];
                    }
                    __syncthreads();
                    nnlm_tile(nn.m, nn_ids, cnt, nn_act, nn_rows);
                }
                for (int i = tid; i < cnt * A; i += NT) {
                    const int e = i / A, c = i - e * A;
                    rows[rb ^ 1][sel_idx[t0 + e] * A + c] = c == 0 ? 0.0f : nn_rows[(size_t)e * Vp + p.sym_word[c]];
                }
                __syncthreads();
            }
            rb ^= 1;
        } else if (has_lm) {
            for (int it = tid; it < nsel * A; it += NT) {
                const int r = it / A, c = it - r * A;
                const int src = NB.prev[r];
                float v;
                if (src >= 0) v = rows[rb][src * A + c];
                else v = c == 0 ? 0.0f : lm_score(p, NB.ctx[r], min(NB.len[r] + 1, ctx_max), (uint32_t)p.sym_word[c]);
                rows[rb ^ 1][it] = v;
            }
            rb ^= 1;
        }
        __syncthreads();
        n = nsel;
        cb ^= 1;
        tc ^= 1;
    }

    // ---- the n best hypotheses through the back-pointers ----------------------------------
    const Beam& B = bm[cb];
    for (int q = tid; q < p.nbest; q += NT) {
        const int64_t o = (int64_t)blockIdx.x * p.nbest + q;
        if (q >= n) {
            p.lens[o] = 0;
            p.scores[o] = -INFINITY;
            continue;
        }
        const int L = B.len[q];
        p.lens[o] = L;
        p.scores[o] = B.key[q];
        int32_t* out = p.ids + p.nbest * u.id_off + (int64_t)q * T;
        int r = q, pos = L - 1;
        for (int t = T - 1; t >= 0 && pos >= 0; --t) {
            const int e = rec[(int64_t)t * K + r];
            const int c = e & 0xFFFF;
            if (c != 0) out[pos--] = c;
            r = e >> 16;
        }
    }
}

__global__ __launch_bounds__(NT) void ctc_beam_kernel(BeamArgs p) { beam_search<false, false, false>(p, NoNNArgs{}); }

__global__ __launch_bounds__(NT) void ctc_lexbeam_kernel(BeamArgs p) { beam_search<true, false, false>(p, NoNNArgs{}); }

__global__ __launch_bounds__(NT) void ctc_nnbeam_kernel(BeamArgs p, NNArgs nn) { beam_search<false, true, false>(p, nn); }

__global__ __launch_bounds__(NT) void ctc_rnnbeam_kernel(BeamArgs p, RNNArgs nn) { beam_search<false, true, true>(p, nn); }

struct BeamPlan {
    std::vector<UttDesc> utt;
    size_t head = 0;     // descriptors + symbol map
    size_t total = 0;
};

// nn_extra: bytes per utterance of the neural LM search (windows, one LM tile) on top of the LM rows
int plan_beam(const sctc_beam_config* cfg, BeamPlan& pl, size_t nn_extra = 0)
{
    SCTC_CHECK_ARG(cfg, "beam: null config");
    SCTC_CHECK_ARG(cfg->B >= 1, "beam: empty batch");
    SCTC_CHECK_ARG(cfg->A >= 2 && cfg->A <= AMAX, "beam: alphabet size %d outside 2..%d", cfg->A, AMAX);
    SCTC_CHECK_ARG(cfg->beam >= 1 && cfg->beam <= KMAX, "beam: beam width %d outside 1..%d", cfg->beam, KMAX);
    SCTC_CHECK_ARG(cfg->nbest >= 1 && cfg->nbest <= cfg->beam, "beam: nbest %d outside 1..beam", cfg->nbest);
    SCTC_CHECK_ARG(cfg->dtype == SCTC_F32 || cfg->dtype == SCTC_F64, "beam: bad dtype %d", cfg->dtype);
    SCTC_CHECK_ARG(cfg->ld >= cfg->A, "beam: ld %lld < A %d", (long long)cfg->ld, cfg->A);
    SCTC_CHECK_ARG(cfg->T_b && cfg->frame_off, "beam: null T_b / frame_off");
    SCTC_CHECK_ARG(isfinite(cfg->alpha) && isfinite(cfg->beta), "beam: alpha / beta not finite");
    if (cfg->lm) {
        SCTC_CHECK_ARG(cfg->sym_word, "beam: an LM needs the symbol -> word map");
        for (int c = 1; c < cfg->A; ++c)
            SCTC_CHECK_ARG(cfg->sym_word[c] >= 1 && cfg->sym_word[c] <= 255,
                           "beam: symbol %d maps to LM word %d outside 1..255", c, cfg->sym_word[c]);
    }
    const int64_t M = (int64_t)cfg->beam * cfg->A;
    const size_t fixed = al256(2 * M * sizeof(float2)) + al256(M * sizeof(uint64_t)) +
                         (cfg->lm || nn_extra ? al256(2 * M * sizeof(float)) : 0) + nn_extra;
    pl.utt.resize(cfg->B);
    pl.head = align256(cfg->B * sizeof(UttDesc)) + align256(AMAX * sizeof(int32_t));
    size_t off = pl.head;
    int64_t id_off = 0;
    for (int b = 0; b < cfg->B; ++b) {
        const int T = cfg->T_b[b];
        SCTC_CHECK_ARG(T >= 0, "beam: utterance %d has %d frames", b, T);
        SCTC_CHECK_ARG(cfg->frame_off[b] >= 0, "beam: utterance %d has a negative frame offset", b);
        UttDesc& d = pl.utt[b];
        d.frame_off = cfg->frame_off[b];
        d.ws_off = (int64_t)off;
        d.id_off = id_off;
        d.T = T;
        d.pad = 0;
        off += fixed + align256((size_t)T * cfg->beam * sizeof(int32_t));
        id_off += T;
    }
    pl.total = off;
    return SCTC_OK;
}

// the lexicon search plans like the character search without an LM: the same workspace
int plan_lexbeam(const sctc_lexbeam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "lexbeam: null config");
    SCTC_CHECK_ARG(cfg->lexicon, "lexbeam: null lexicon");
    SCTC_CHECK_ARG(cfg->A == cfg->lexicon->A, "lexbeam: alphabet size %d, the lexicon was built for %d", cfg->A,
                   cfg->lexicon->A);
    SCTC_CHECK_ARG(cfg->space >= 1 && cfg->space < cfg->A, "lexbeam: space symbol %d outside 1..A-1", cfg->space);
    sctc_beam_config c{};
    c.B = cfg->B;
    c.A = cfg->A;
    c.dtype = cfg->dtype;
    c.beam = cfg->beam;
    c.nbest = cfg->nbest;
    c.ld = cfg->ld;
    c.T_b = cfg->T_b;
    c.frame_off = cfg->frame_off;
    c.alpha = cfg->alpha;
    c.beta = cfg->beta;
    return plan_beam(&c, pl);
}

// the neural LM search plans like the character search with an LM, plus its windows and LM tile
int plan_nnbeam(const sctc_nnbeam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "nnbeam: null config");
    SCTC_CHECK_ARG(cfg->lm, "nnbeam: null LM");
    SCTC_CHECK_ARG(cfg->sym_word, "nnbeam: null symbol -> LM id map");
    SCTC_CHECK_ARG(cfg->A >= 2 && cfg->A <= AMAX, "nnbeam: alphabet size %d outside 2..%d", cfg->A, AMAX);
    SCTC_CHECK_ARG(cfg->beam >= 1 && cfg->beam <= KMAX, "nnbeam: beam width %d outside 1..%d", cfg->beam, KMAX);
    const NNLMDev& m = cfg->lm->dev;
    for (int c = 1; c < cfg->A; ++c)
        SCTC_CHECK_ARG(cfg->sym_word[c] >= 0 && cfg->sym_word[c] < m.V,
                       "nnbeam: symbol %d maps to LM id %d outside 0..%d", c, cfg->sym_word[c], m.V - 1);
    sctc_beam_config c{};
    c.B = cfg->B;
    c.A = cfg->A;
    c.dtype = cfg->dtype;
    c.beam = cfg->beam;
    c.nbest = cfg->nbest;
    c.ld = cfg->ld;
    c.T_b = cfg->T_b;
    c.frame_off = cfg->frame_off;
    c.alpha = cfg->alpha;
    c.beta = cfg->beta;
    return plan_beam(&c, pl, al256((size_t)2 * cfg->beam * WIN) + nn_tile_bytes(m.hmax, m.Vp, m.K));
}

// the recurrent LM search plans like the character search with an LM, plus the states of both beams
// and its LM tile
int plan_rnnbeam(const sctc_rnnbeam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "rnnbeam: null config");
    SCTC_CHECK_ARG(cfg->lm, "rnnbeam: null LM");
    SCTC_CHECK_ARG(cfg->sym_word, "rnnbeam: null symbol -> LM id map");
    SCTC_CHECK_ARG(cfg->A >= 2 && cfg->A <= AMAX, "rnnbeam: alphabet size %d outside 2..%d", cfg->A, AMAX);
    SCTC_CHECK_ARG(cfg->beam >= 1 && cfg->beam <= KMAX, "rnnbeam: beam width %d outside 1..%d", cfg->beam, KMAX);
    const RNNLMDev& m = cfg->lm->dev;
    for (int c = 1; c < cfg->A; ++c)
        SCTC_CHECK_ARG(cfg->sym_word[c] >= 0 && cfg->sym_word[c] < m.V,
                       "rnnbeam: symbol %d maps to LM id %d outside 0..%d", c, cfg->sym_word[c], m.V - 1);
    sctc_beam_config c{};
    c.B = cfg->B;
    c.A = cfg->A;
    c.dtype = cfg->dtype;
    c.beam = cfg->beam;
    c.nbest = cfg->nbest;
    c.ld = cfg->ld;
    c.T_b = cfg->T_b;
    c.frame_off = cfg->frame_off;
    c.alpha = cfg->alpha;
    c.beta = cfg->beta;
    return plan_beam(&c, pl, al256((size_t)2 * cfg->beam * m.H * sizeof(float)) + rnn_tile_bytes(m.H, m.Vp));
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_lm_create(const uint64_t* keys_host, const float* prob_host, const float* backoff_host,
                   int64_t capacity, int32_t order, int32_t bos_word, sctc_lm_t* out)
{
    SCTC_CHECK_ARG(out && keys_host && prob_host && backoff_host, "lm: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(capacity >= 2 && (capacity & (capacity - 1)) == 0, "lm: capacity %lld not a power of two",
                   (long long)capacity);
    SCTC_CHECK_ARG(order >= 1 && order <= 8, "lm: order %d outside 1..8", order);
    SCTC_CHECK_ARG(bos_word >= 1 && bos_word <= 255, "lm: <s> word id %d outside 1..255", bos_word);
    int64_t used = 0;
    for (int64_t i = 0; i < capacity; ++i) used += keys_host[i] != 0;
    SCTC_CHECK_ARG(used < capacity, "lm: table without an empty slot");
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    sctc_lm* lm = new sctc_lm();
    const size_t kb = capacity * sizeof(uint64_t), fb = capacity * sizeof(float);
    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, kb + 2 * fb);
    if (e == hipSuccess) e = hipMemcpy(mem, keys_host, kb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)mem + kb, prob_host, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)mem + kb + fb, backoff_host, fb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        delete lm;
        return set_error(SCTC_ERR_HIP, "lm: upload failed: %s", hipGetErrorString(e));
    }
    lm->key = (uint64_t*)mem;
    lm->prob = (float*)((char*)mem + kb);
    lm->bo = (float*)((char*)mem + kb + fb);
    lm->cap = capacity;
    lm->order = order;
    lm->bos = bos_word;
    lm->device = dev;
    *out = lm;
    return SCTC_OK;
}

int sctc_lm_destroy(sctc_lm_t lm)
{
    if (!lm) return SCTC_OK;
    if (lm->key) (void)hipFree(lm->key);
    delete lm;
    return SCTC_OK;
}

size_t sctc_ctc_beam_workspace_bytes(const sctc_beam_config* cfg)
{
    BeamPlan pl;
    if (plan_beam(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_beam_decode_batch(const sctc_beam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                               int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_beam(cfg, pl));
    SCTC_CHECK_ARG(probs_dev && lengths_dev && scores_dev && workspace_dev, "beam: null device pointer");
    int64_t total_T = 0;
    for (int b = 0; b < cfg->B; ++b) total_T += cfg->T_b[b];
    SCTC_CHECK_ARG(ids_dev || total_T == 0, "beam: null ids");
    if (workspace_bytes < pl.total)
        return set_error(SCTC_ERR_WORKSPACE, "beam: workspace %zu bytes < %zu needed", workspace_bytes, pl.total);
    hipStream_t s = (hipStream_t)stream;
    std::vector<char> head(pl.head, 0);
    memcpy(head.data(), pl.utt.data(), cfg->B * sizeof(UttDesc));
    const size_t sym_off = align256(cfg->B * sizeof(UttDesc));
    if (cfg->lm) memcpy(head.data() + sym_off, cfg->sym_word, cfg->A * sizeof(int32_t));
    // small and synchronous with respect to the host buffer: a plain copy, then the launch
    SCTC_HIP_TRY(hipMemcpyAsync(workspace_dev, head.data(), pl.head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(hipStreamSynchronize(s));

    BeamArgs a{};
    a.probs = probs_dev;
    a.ld = cfg->ld;
    a.f64 = cfg->dtype == SCTC_F64;
    a.A = cfg->A;
    a.K = cfg->beam;
    a.nbest = cfg->nbest;
    a.alpha = cfg->alpha;
    a.beta = cfg->beta;
    a.utt = (const UttDesc*)workspace_dev;
    a.sym_word = (const int32_t*)((char*)workspace_dev + sym_off);
    a.ws = (char*)workspace_dev;
    if (cfg->lm) {
        a.lm_key = cfg->lm->key;
        a.lm_prob = cfg->lm->prob;
        a.lm_bo = cfg->lm->bo;
        a.lm_mask = (uint64_t)(cfg->lm->cap - 1);
        a.lm_order = cfg->lm->order;
        a.lm_bos = cfg->lm->bos;
    }
    a.ids = ids_dev;
    a.lens = lengths_dev;
    a.scores = scores_dev;
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(cfg->B), dim3(NT), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"

extern "C" {

int sctc_lexicon_create(const int32_t* child_host, const int32_t* word_host, int64_t nodes, int32_t A,
                        int32_t space, const float* ug_prob_host, const float* ug_backoff_host, int64_t n_words,
                        const uint64_t* bg_keys_host, const float* bg_vals_host, int64_t bg_capacity,
                        int32_t start_word, sctc_lexicon_t* out)
{
    SCTC_CHECK_ARG(out, "lexicon: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(child_host && word_host && ug_prob_host && ug_backoff_host && bg_keys_host && bg_vals_host,
                   "lexicon: null argument");
    SCTC_CHECK_ARG(A >= 2 && A <= AMAX, "lexicon: alphabet size %d outside 2..%d", A, AMAX);
    SCTC_CHECK_ARG(space >= 1 && space < A, "lexicon: space symbol %d outside 1..A-1", space);
    SCTC_CHECK_ARG(nodes >= 1 && nodes <= (int64_t)INT32_MAX / A, "lexicon: %lld nodes outside 1..2^31/A",
                   (long long)nodes);
    SCTC_CHECK_ARG(n_words >= 1 && n_words <= INT32_MAX, "lexicon: %lld words", (long long)n_words);
    SCTC_CHECK_ARG(start_word >= 0 && start_word < n_words, "lexicon: <s> word id %d outside the vocabulary",
                   start_word);
    SCTC_CHECK_ARG(bg_capacity >= 2 && (bg_capacity & (bg_capacity - 1)) == 0,
                   "lexicon: bigram capacity %lld not a power of two", (long long)bg_capacity);
    // everything the kernel follows without a check of its own is checked here, once
    SCTC_CHECK_ARG(word_host[0] < 0, "lexicon: the root is a word");
    for (int64_t n = 0; n < nodes; ++n) {
        SCTC_CHECK_ARG(word_host[n] >= -1 && word_host[n] < n_words, "lexicon: node %lld has word id %d", (long long)n,
                       word_host[n]);
        SCTC_CHECK_ARG(child_host[n * A] < 0 && child_host[n * A + space] < 0,
                       "lexicon: node %lld has a child for the blank or the space", (long long)n);
        for (int c = 1; c < A; ++c) {
            const int32_t ch = child_host[n * A + c];
            SCTC_CHECK_ARG(ch >= -1 && ch < nodes && ch != 0, "lexicon: node %lld symbol %d -> node %d", (long long)n, c, ch);
        }
    }
    int64_t used = 0;
    for (int64_t i = 0; i < bg_capacity; ++i) {
        const uint64_t k = bg_keys_host[i];
        if (k == BG_EMPTY) continue;
        ++used;
        SCTC_CHECK_ARG((int64_t)(k >> 32) < n_words && (int64_t)(k & 0xFFFFFFFFull) < n_words,
                       "lexicon: bigram slot %lld names a word outside the vocabulary", (long long)i);
    }
    SCTC_CHECK_ARG(used < bg_capacity, "lexicon: bigram table without an empty slot");
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    const size_t sz[6] = {al256((size_t)nodes * A * sizeof(int32_t)), al256((size_t)nodes * sizeof(int32_t)),
                          al256((size_t)n_words * sizeof(float)),     al256((size_t)n_words * sizeof(float)),
                          al256((size_t)bg_capacity * sizeof(uint64_t)), al256((size_t)bg_capacity * sizeof(float))};
    const size_t raw[6] = {(size_t)nodes * A * sizeof(int32_t), (size_t)nodes * sizeof(int32_t),
                           (size_t)n_words * sizeof(float),     (size_t)n_words * sizeof(float),
                           (size_t)bg_capacity * sizeof(uint64_t), (size_t)bg_capacity * sizeof(float)};
    const void* src[6] = {child_host, word_host, ug_prob_host, ug_backoff_host, bg_keys_host, bg_vals_host};
    size_t total = 0, off[6];
    for (int i = 0; i < 6; ++i) {
        off[i] = total;
        total += sz[i];
    }
    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, total);
    for (int i = 0; i < 6 && e == hipSuccess; ++i)
        e = hipMemcpy((char*)mem + off[i], src[i], raw[i], hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        return set_error(SCTC_ERR_HIP, "lexicon: upload failed: %s", hipGetErrorString(e));
    }
    sctc_lexicon* lx = new sctc_lexicon();
    lx->mem = (char*)mem;
    lx->child = (int32_t*)(lx->mem + off[0]);
    lx->word = (int32_t*)(lx->mem + off[1]);
    lx->ug = (float*)(lx->mem + off[2]);
    lx->bo = (float*)(lx->mem + off[3]);
    lx->bg_key = (uint64_t*)(lx->mem + off[4]);
    lx->bg_val = (float*)(lx->mem + off[5]);
    lx->nodes = nodes;
    lx->n_words = n_words;
    lx->bg_cap = bg_capacity;
    lx->bytes = total;
    lx->A = A;
    lx->start = start_word;
    lx->device = dev;
    *out = lx;
    return SCTC_OK;
}

int sctc_lexicon_destroy(sctc_lexicon_t lexicon)
{
    if (!lexicon) return SCTC_OK;
    if (lexicon->mem) (void)hipFree(lexicon->mem);
    delete lexicon;
    return SCTC_OK;
}

size_t sctc_lexicon_bytes(sctc_lexicon_t lexicon) { return lexicon ? lexicon->bytes : 0; }

size_t sctc_ctc_lexbeam_workspace_bytes(const sctc_lexbeam_config* cfg)
{
    BeamPlan pl;
    if (plan_lexbeam(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_lexbeam_decode_batch(const sctc_lexbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                  int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_lexbeam(cfg, pl));
    SCTC_CHECK_ARG(probs_dev && lengths_dev && scores_dev && workspace_dev, "lexbeam: null device pointer");
    int64_t total_T = 0;
    for (int b = 0; b < cfg->B; ++b) total_T += cfg->T_b[b];
    SCTC_CHECK_ARG(ids_dev || total_T == 0, "lexbeam: null ids");
    if (workspace_bytes < pl.total)
        return set_error(SCTC_ERR_WORKSPACE, "lexbeam: workspace %zu bytes < %zu needed", workspace_bytes, pl.total);
    hipStream_t s = (hipStream_t)stream;
    std::vector<char> head(pl.head, 0);
    memcpy(head.data(), pl.utt.data(), cfg->B * sizeof(UttDesc));
    SCTC_HIP_TRY(hipMemcpyAsync(workspace_dev, head.data(), pl.head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(hipStreamSynchronize(s));

    const sctc_lexicon* lx = cfg->lexicon;
    BeamArgs a{};
    a.probs = probs_dev;
    a.ld = cfg->ld;
    a.f64 = cfg->dtype == SCTC_F64;
    a.A = cfg->A;
    a.K = cfg->beam;
    a.nbest = cfg->nbest;
    a.alpha = cfg->alpha;
    a.beta = cfg->beta;
    a.utt = (const UttDesc*)workspace_dev;
    a.ws = (char*)workspace_dev;
    a.ids = ids_dev;
    a.lens = lengths_dev;
    a.scores = scores_dev;
    a.lx_child = lx->child;
    a.lx_word = lx->word;
    a.lx_ug = lx->ug;
    a.lx_bo = lx->bo;
    a.lx_key = lx->bg_key;
    a.lx_val = lx->bg_val;
    a.lx_mask = (uint64_t)(lx->bg_cap - 1);
    a.lx_start = lx->start;
    a.space = cfg->space;
    hipLaunchKernelGGL(ctc_lexbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"

extern "C" {

size_t sctc_ctc_nnbeam_workspace_bytes(const sctc_nnbeam_config* cfg)
{
    BeamPlan pl;
    if (plan_nnbeam(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_nnbeam_decode_batch(const sctc_nnbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                 int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_nnbeam(cfg, pl));
    SCTC_CHECK_ARG(probs_dev && lengths_dev && scores_dev && workspace_dev, "nnbeam: null device pointer");
    int64_t total_T = 0;
    for (int b = 0; b < cfg->B; ++b) total_T += cfg->T_b[b];
    SCTC_CHECK_ARG(ids_dev || total_T == 0, "nnbeam: null ids");
    if (workspace_bytes < pl.total)
        return set_error(SCTC_ERR_WORKSPACE, "nnbeam: workspace %zu bytes < %zu needed", workspace_bytes, pl.total);
    hipStream_t s = (hipStream_t)stream;
    std::vector<char> head(pl.head, 0);
    memcpy(head.data(), pl.utt.data(), cfg->B * sizeof(UttDesc));
    const size_t sym_off = align256(cfg->B * sizeof(UttDesc));
    memcpy(head.data() + sym_off, cfg->sym_word, cfg->A * sizeof(int32_t));
    ((int32_t*)(head.data() + sym_off))[0] = 0;        // the blank has no LM id; never read
    SCTC_HIP_TRY(hipMemcpyAsync(workspace_dev, head.data(), pl.head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(hipStreamSynchronize(s));

    BeamArgs a{};
    a.probs = probs_dev;
    a.ld = cfg->ld;
    a.f64 = cfg->dtype == SCTC_F64;
    a.A = cfg->A;
    a.K = cfg->beam;
    a.nbest = cfg->nbest;
    a.alpha = cfg->alpha;
    a.beta = cfg->beta;
    a.utt = (const UttDesc*)workspace_dev;
    a.sym_word = (const int32_t*)((char*)workspace_dev + sym_off);
    a.ws = (char*)workspace_dev;
    a.ids = ids_dev;
    a.lens = lengths_dev;
    a.scores = scores_dev;
    NNArgs nn{};
    nn.m = cfg->lm->dev;
    hipLaunchKernelGGL(ctc_nnbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a, nn);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"

extern "C" {

size_t sctc_ctc_rnnbeam_workspace_bytes(const sctc_rnnbeam_config* cfg)
{
    BeamPlan pl;
    if (plan_rnnbeam(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_rnnbeam_decode_batch(const sctc_rnnbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                  int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_rnnbeam(cfg, pl));
    SCTC_CHECK_ARG(probs_dev && lengths_dev && scores_dev && workspace_dev, "rnnbeam: null device pointer");
    int64_t total_T = 0;
    for (int b = 0; b < cfg->B; ++b) total_T += cfg->T_b[b];
    SCTC_CHECK_ARG(ids_dev || total_T == 0, "rnnbeam: null ids");
    if (workspace_bytes < pl.total)
        return set_error(SCTC_ERR_WORKSPACE, "rnnbeam: workspace %zu bytes < %zu needed", workspace_bytes, pl.total);
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    SCTC_CHECK_ARG(dev == cfg->lm->device, "rnnbeam: the LM lives on device %d, the current device is %d",
                   cfg->lm->device, dev);
    hipStream_t s = (hipStream_t)stream;
    std::vector<char> head(pl.head, 0);
    memcpy(head.data(), pl.utt.data(), cfg->B * sizeof(UttDesc));
    const size_t sym_off = align256(cfg->B * sizeof(UttDesc));
    memcpy(head.data() + sym_off, cfg->sym_word, cfg->A * sizeof(int32_t));
    ((int32_t*)(head.data() + sym_off))[0] = 0;        // the blank has no LM id; never read
    SCTC_HIP_TRY(hipMemcpyAsync(workspace_dev, head.data(), pl.head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(hipStreamSynchronize(s));

    BeamArgs a{};
    a.probs = probs_dev;
    a.ld = cfg->ld;
    a.f64 = cfg->dtype == SCTC_F64;
    a.A = cfg->A;
    a.K = cfg->beam;
    a.nbest = cfg->nbest;
    a.alpha = cfg->alpha;
    a.beta = cfg->beta;
    a.utt = (const UttDesc*)workspace_dev;
    a.sym_word = (const int32_t*)((char*)workspace_dev + sym_off);
    a.ws = (char*)workspace_dev;
    a.ids = ids_dev;
    a.lens = lengths_dev;
    a.scores = scores_dev;
    RNNArgs nn{};
    nn.m = cfg->lm->dev;
    nn.state_copies = 1;
    if (const char* e = getenv("SCTC_RNNBEAM_STATE_COPIES")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 4) nn.state_copies = v;
    }
    hipLaunchKernelGGL(ctc_rnnbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a, nn);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
