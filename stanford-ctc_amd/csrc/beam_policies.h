// The LM policies of the prefix beam search (beam_search.h lists the hooks); the search with a character
// n-gram LM, or none, is written out in beam_ngram.h:
//   LexiconPolicy  a prefix tree of words with a word-bigram LM (the reference's
//                  ctc_fast/decoder/bg_decoder.pyx:18-95) -- §4.6
//   LexiconNgramPolicy  the same tree with a word n-gram LM of order 2..5 -- §4.6b
//   NNPolicy       a window neural LM supplies the rows (the lexicon-free path of the reference's
//                  ctc_fast/decoder/clm_decoder2.pyx), through nnlm_tile, the routine sctc_nnlm_rows runs -- §4.7
//   RNNPolicy      a recurrent neural LM supplies them (the `rnn` model type of clm_decoder2.pyx), through
//                  rnnlm_tile, the routine sctc_rnnlm_step runs -- §4.10
// Each owns its kernel-argument struct, its part of the workspace and its per-entry state.
#pragma once
#include "beam_search.h"
#include "nnlm_dev.h"
#include "rnnlm_dev.h"

namespace sctc {
namespace beam {

struct NoState {
};

// A pair of buffers, one per beam: step 4 fills `nxt` from `cur` and flips them.  (Two named pointers, not
// an array indexed by the beam's parity: the policy object has to dissolve into registers.)
template <typename T>
struct BeamPair {
    T* cur;
    T* nxt;
    __device__ __forceinline__ void carve(char* w, size_t count)
    {
        cur = (T*)w;
        nxt = (T*)w + count;
    }
    __device__ __forceinline__ void flip()
    {
        T* t = cur;
        cur = nxt;
        nxt = t;
    }
};

// What the neural policies share: rows.cur[r * A + c] = log10 P(c | prefix of entry r), every
// extension a candidate, the bonus on the symbols, no per-entry LDS state
struct LmRows {
    using State = NoState;
    BeamPair<float> rows;

    __device__ __forceinline__ bool candidate(const BeamArgs&, const State&, int, int) const { return true; }
    __device__ __forceinline__ int counted_len(const BeamArgs&, const Beam& B, const State&, int j, int c) const
    {
        return c == 0 ? B.len[j] : B.len[j] + 1;
    }

    __device__ __forceinline__ char* carve_rows(char* w, const BeamArgs& p)
    {
        const int64_t M = (int64_t)p.K * p.A;
        rows.carve(w, M);
        return w + align256(2 * M * sizeof(float));
    }
    __device__ __forceinline__ double row_term(const BeamArgs& p, int e, int c) const
    {
        return p.alpha * (double)rows.cur[e * p.A + c];
    }
};

// ---- lexicon with a word-bigram LM -----------------------------------------------------------------

struct LexiconArgs {
    const int32_t* child;
    const int32_t* word;
    const float* ug;
    const float* bo;
    const uint64_t* key;
    const float* val;
    uint64_t mask;
    int32_t start, space;
};

// per beam entry of the lexicon search; a function of the prefix alone
struct LexState {
    int32_t node[KMAX];   // prefix-tree node the unfinished word has reached (0 = root)
    int32_t pw[KMAX];     // id of the last finished word (<s> at the start)
    int32_t nw[KMAX];     // finished words
    int32_t wd[KMAX];     // word id of `node`, -1: a space cannot follow
    float bg[KMAX];       // bg_prob(pw, wd): the LM value of the space extension, 0 without one
};

// bg_prob(w1, w2) of fastdecode/lm.cpp:119-127: the listed bigram, or -- when there is none or it
// is exactly 0 -- the float32 sum back-off(w1) + unigram(w2)
__device__ inline float lex_bg(const LexiconArgs& a, int w1, int w2)
{
    const uint64_t key = ((uint64_t)(uint32_t)w1 << 32) | (uint32_t)w2;
    uint64_t s = mix64(key) & a.mask;
    float v = 0.0f;
    while (true) {
        const uint64_t k = a.key[s];
        if (k == key) {
            v = a.val[s];
            break;
        }
        if (k == BG_EMPTY) break;
        s = (s + 1) & a.mask;
    }
    if (v == 0.0f) v = a.bo[w1] + a.ug[w2];
    return v;
}

// no rows and no workspace of its own: the LM value of the one extension that has one, the space, is
// cached per entry
struct LexiconPolicy {
    using Args = LexiconArgs;
    using State = LexState;
    const Args& a;

    __device__ __forceinline__ LexiconPolicy(const BeamArgs&, const Args& args) : a(args) {}
    __device__ __forceinline__ char* carve(char* w, const BeamArgs&) { return w; }
    __device__ __forceinline__ void empty_entry(const BeamArgs&, Beam&, State& x0)
    {
        x0.node[0] = 0;
        x0.pw[0] = a.start;
        x0.nw[0] = 0;
        x0.wd[0] = a.word[0];
        x0.bg[0] = 0.0f;
    }
    __device__ __forceinline__ void empty_rows(const BeamArgs&, const Beam&) {}
    // a space only after a whole word, a letter only along the tree: anything else is no candidate
    // (bg_decoder.pyx:48-61)
    __device__ __forceinline__ bool candidate(const BeamArgs& p, const State& X, int j, int c) const
    {
        return c == a.space ? X.wd[j] >= 0 : a.child[(int64_t)X.node[j] * p.A + c] >= 0;
    }
    __device__ __forceinline__ double lm_term(const BeamArgs& p, const State& X, int e, int c) const
    {
        return c == a.space ? p.alpha * (double)X.bg[e] : 0.0;
    }
    __device__ __forceinline__ int counted_len(const BeamArgs&, const Beam&, const State& X, int j, int c) const
    {
        return c == 0 ? X.nw[j] : X.nw[j] + (c == a.space);
    }
    __device__ __forceinline__ void carry(const BeamArgs&, const Beam&, Beam&, const State& X, State& NX, int j, int r)
    {
        NX.node[r] = X.node[j];
        NX.pw[r] = X.pw[j];
        NX.nw[r] = X.nw[j];
        NX.wd[r] = X.wd[j];
        NX.bg[r] = X.bg[j];
    }
    __device__ __forceinline__ void extend(const BeamArgs& p, const Beam&, Beam&, const State& X, State& NX, int j, int c,
                                           int r)
    {
        const bool sp = c == a.space;
        const int nd = sp ? 0 : a.child[(int64_t)X.node[j] * p.A + c];
        const int pw = sp ? X.wd[j] : X.pw[j];
        const int wd = a.word[nd];
        NX.node[r] = nd;
        NX.pw[r] = pw;
        NX.nw[r] = X.nw[j] + sp;
        NX.wd[r] = wd;
        NX.bg[r] = wd >= 0 ? lex_bg(a, pw, wd) : 0.0f;
    }
    __device__ __forceinline__ void new_rows(const BeamArgs&, const Beam&, int, int, const FrameScratch&) {}
};

// ---- lexicon with a word n-gram LM of order 2..5 (§4.6b) --------------------------------------------

struct LexiconNgramArgs {
    const int32_t* child;
    const int32_t* word;
    const float* ug;
    const float* bo;
    const uint64_t* key;   // (context id << 32) | w of every listed n-gram of length >= 2, all ones = empty
    const float* val;
    const float* nbo;      // the n-gram's own back-off
    const int32_t* id;     // the n-gram's id as a context, -1 at full order
    uint64_t mask;
    int32_t start, space, order;
};

constexpr int NG_HIST = NG_MAX_ORDER - 1;   // history ids of the highest order

// per beam entry; a function of the prefix alone.  The history is the last min(order - 1, finished words + 1)
// word ids of <s> + the finished words, newest first, -1 beyond its length.
struct LexNgState {
    int32_t node[KMAX];   // prefix-tree node the unfinished word has reached (0 = root)
    int32_t nw[KMAX];     // finished words
    int32_t wd[KMAX];     // word id of `node`, -1: a space cannot follow
    float lm[KMAX];       // P(wd | history): the LM value of the space extension, 0 without one
    int32_t h0[KMAX], h1[KMAX], h2[KMAX], h3[KMAX];
};

// slot of the listed n-gram (context, w), -1 for none; ends at the table's empty slot
__device__ inline int64_t ng_find(const LexiconNgramArgs& a, int ctx, int w)
{
    const uint64_t key = ((uint64_t)(uint32_t)ctx << 32) | (uint32_t)w;
    uint64_t s = mix64(key) & a.mask;
    while (true) {
        const uint64_t k = a.key[s];
        if (k == key) return (int64_t)s;
        if (k == BG_EMPTY) return -1;
        s = (s + 1) & a.mask;
    }
}

// P(w | h) by the ARPA back-off rule in kenlm's order of float32 additions (arpa_lm.ArpaLM.score_ids; the
// host twin is decoder/ngram_lm.py walk_packed).  Per context length m: the id of the history's suffix of
// that length by chaining from its oldest word -- a miss means the suffix is not listed, and then neither
// is any n-gram it begins (the loader requires every listed n-gram's prefix) -- then (suffix, w) while the
// match holds, and the suffix's back-off from the first miss on.  Both stop at the first suffix that is not
// listed.  h is indexed by constants only, so it stays in registers.
__device__ __forceinline__ float lex_ng(const LexiconNgramArgs& a, const int32_t (&h)[NG_HIST], int w)
{
    float p = a.ug[w];
    bool matching = true, open = true;
#pragma unroll
    for (int m = 1; m <= NG_HIST; ++m) {
        open = open && h[m - 1] >= 0;
        int cid = open ? h[m - 1] : 0;
        float cbo = m == 1 ? a.bo[cid] : 0.0f;
#pragma unroll
        for (int i = m - 2; i >= 0; --i) {
            if (open) {
                const int64_t s = ng_find(a, cid, h[i]);
                if (s < 0) {
                    open = false;
                } else {
                    cid = a.id[s];
                    cbo = a.nbo[s];
                }
            }
        }
        if (open) {
            int64_t s = -1;
            if (matching) s = ng_find(a, cid, w);
            if (s >= 0) {
                p = a.val[s];
            } else {
                matching = false;
                p += cbo;
            }
        }
    }
    return p;
}

// LexiconPolicy with the history of an n-gram in place of the previous word
struct LexiconNgramPolicy {
    using Args = LexiconNgramArgs;
    using State = LexNgState;
    const Args& a;

    __device__ __forceinline__ LexiconNgramPolicy(const BeamArgs&, const Args& args) : a(args) {}
    __device__ __forceinline__ char* carve(char* w, const BeamArgs&) { return w; }
    __device__ __forceinline__ void empty_entry(const BeamArgs&, Beam&, State& x0)
    {
        x0.node[0] = 0;
        x0.nw[0] = 0;
        x0.wd[0] = a.word[0];
        x0.lm[0] = 0.0f;
        x0.h0[0] = a.start;
        x0.h1[0] = -1;
        x0.h2[0] = -1;
        x0.h3[0] = -1;
    }
    __device__ __forceinline__ void empty_rows(const BeamArgs&, const Beam&) {}
    __device__ __forceinline__ bool candidate(const BeamArgs& p, const State& X, int j, int c) const
    {
        return c == a.space ? X.wd[j] >= 0 : a.child[(int64_t)X.node[j] * p.A + c] >= 0;
    }
    __device__ __forceinline__ double lm_term(const BeamArgs& p, const State& X, int e, int c) const
    {
        return c == a.space ? p.alpha * (double)X.lm[e] : 0.0;
    }
    __device__ __forceinline__ int counted_len(const BeamArgs&, const Beam&, const State& X, int j, int c) const
    {
        return c == 0 ? X.nw[j] : X.nw[j] + (c == a.space);
    }
    __device__ __forceinline__ void carry(const BeamArgs&, const Beam&, Beam&, const State& X, State& NX, int j, int r)
    {
        NX.node[r] = X.node[j];
        NX.nw[r] = X.nw[j];
        NX.wd[r] = X.wd[j];
        NX.lm[r] = X.lm[j];
        NX.h0[r] = X.h0[j];
        NX.h1[r] = X.h1[j];
        NX.h2[r] = X.h2[j];
        NX.h3[r] = X.h3[j];
    }
    // a space appends the finished word to the history and drops what is older than order - 1 words
    __device__ __forceinline__ void extend(const BeamArgs& p, const Beam&, Beam&, const State& X, State& NX, int j, int c,
                                           int r)
    {
        const bool sp = c == a.space;
        const int nd = sp ? 0 : a.child[(int64_t)X.node[j] * p.A + c];
        const int wd = a.word[nd];
        int32_t h[NG_HIST] = {X.h0[j], X.h1[j], X.h2[j], X.h3[j]};
        static_assert(NG_HIST == 4, "the history is four named arrays");
        if (sp) {
            h[3] = a.order > 4 ? h[2] : -1;
            h[2] = a.order > 3 ? h[1] : -1;
            h[1] = a.order > 2 ? h[0] : -1;
            h[0] = X.wd[j];
        }
        NX.node[r] = nd;
        NX.nw[r] = X.nw[j] + sp;
        NX.wd[r] = wd;
        NX.h0[r] = h[0];
        NX.h1[r] = h[1];
        NX.h2[r] = h[2];
        NX.h3[r] = h[3];
        NX.lm[r] = wd >= 0 ? lex_ng(a, h, wd) : 0.0f;
    }
    __device__ __forceinline__ void new_rows(const BeamArgs&, const Beam&, int, int, const FrameScratch&) {}
};

// ---- the two neural LMs ----------------------------------------------------------------------------

// Step 4 of a neural policy: the carried entries copy their rows (and whatever else the policy carries
// cooperatively), the new entries are compacted in rank order and evaluated NN_TILE to a tile --
// run_tile fills the tile from entries sel_idx[t0 .. t0 + cnt) and runs the LM -- and the tile's rows
// are scattered through sym_word.
template <typename P>
__device__ __forceinline__ void neural_rows(P& pol, const BeamArgs& p, const Beam& NB, int nsel, int t,
                                            const FrameScratch& f)
{
    const int tid = threadIdx.x, A = p.A;
    for (int it = tid; it < nsel * A; it += NT) {
        const int r = it / A;
        const int src = NB.prev[r];
        if (src >= 0) pol.rows.nxt[it] = pol.rows.cur[src * A + (it - r * A)];
    }
    pol.carry_shared(NB, nsel);
    // the new entries in rank order, 32 to a tile (sel_idx is free until the next select)
    const int fresh = tid < nsel && NB.prev[tid] < 0;
    int n_new;
    const int pos = block_excl_scan(fresh, f.scan, &n_new);
    if (fresh) f.sel_idx[pos] = tid;
    __syncthreads();
    const int Vp = pol.a.m.Vp;
    for (int t0 = 0; t0 < n_new; t0 += NN_TILE) {
        const int cnt = min(NN_TILE, n_new - t0);
        pol.run_tile(p, f.sel_idx + t0, cnt, t, f);
        for (int i = tid; i < cnt * A; i += NT) {
            const int e = i / A, c = i - e * A;
            pol.rows.nxt[f.sel_idx[t0 + e] * A + c] = c == 0 ? 0.0f : pol.tile_rows[(size_t)e * Vp + p.sym_word[c]];
        }
        __syncthreads();
    }
    pol.flip();
}

// what both neural policies are: rows with the row's term for every extension, and the scratch of one LM tile
struct NeuralRows : LmRows {
    float* tile_act;    // the LM tile's activations
    float* tile_rows;   // its rows, [NN_TILE][Vp]

    __device__ __forceinline__ void empty_entry(const BeamArgs&, Beam&, State&) {}
    __device__ __forceinline__ double lm_term(const BeamArgs& p, const State&, int e, int c) const { return row_term(p, e, c); }
    // the row of the empty prefix, from slot 0 of the tile
    __device__ __forceinline__ void first_row(const BeamArgs& p)
    {
        for (int c = threadIdx.x; c < p.A; c += NT) rows.cur[c] = c == 0 ? 0.0f : tile_rows[p.sym_word[c]];
    }
};

struct NNArgs {
    NNLMDev m;
};
constexpr int WIN = NN_MAX_CONTEXT;   // bytes of a beam entry's context window (one LM id per byte)

// every beam entry carries the window of the last K LM ids of <null>.. <s> + P, copied from its parent
// and shifted on extension
struct NNPolicy : NeuralRows {
    using Args = NNArgs;
    const Args& a;
    BeamPair<uint8_t> win;   // the context windows, [K][WIN]
    int32_t* tile_ids;   // the windows of one tile as nnlm_tile reads them

    __device__ __forceinline__ NNPolicy(const BeamArgs&, const Args& args) : a(args) {}
    __device__ __forceinline__ char* carve(char* w, const BeamArgs& p)
    {
        w = carve_rows(w, p);
        win.carve(w, (size_t)p.K * WIN);
        w += align256((size_t)2 * p.K * WIN);
        tile_act = (float*)w;
        tile_rows = (float*)(w + nn_act_bytes(a.m.hmax));
        tile_ids = (int32_t*)(w + nn_act_bytes(a.m.hmax) + nn_row_bytes(a.m.Vp));
        return w + nn_tile_bytes(a.m.hmax, a.m.Vp, a.m.K);
    }
    // the empty prefix: <null> .. <null> <s>
    __device__ __forceinline__ void empty_rows(const BeamArgs& p, const Beam&)
    {
        const int CK = a.m.K;
        for (int s = threadIdx.x; s < CK; s += NT) {
            const int id = s == CK - 1 ? a.m.bos : a.m.null_id;
            win.cur[s] = (uint8_t)id;
            tile_ids[s] = id;
        }
        __syncthreads();
        nnlm_tile(a.m, tile_ids, 1, tile_act, tile_rows);
        first_row(p);
    }
    __device__ __forceinline__ void carry(const BeamArgs&, const Beam&, Beam&, const State&, State&, int j, int r)
    {
        const uint4* src = (const uint4*)(win.cur + (size_t)j * WIN);
        uint4* dst = (uint4*)(win.nxt + (size_t)r * WIN);
        dst[0] = src[0];
        dst[1] = src[1];
    }
    // the parent's window, one slot older, and the new symbol's LM id
    __device__ __forceinline__ void extend(const BeamArgs& p, const Beam&, Beam&, const State&, State&, int j, int c, int r)
    {
        const uint8_t* src = win.cur + (size_t)j * WIN;
        uint8_t* dst = win.nxt + (size_t)r * WIN;
        const int CK = a.m.K;
        for (int s = 0; s + 1 < CK; ++s) dst[s] = src[s + 1];
        dst[CK - 1] = (uint8_t)p.sym_word[c];
    }
    __device__ __forceinline__ void carry_shared(const Beam&, int) {}
    __device__ __forceinline__ void run_tile(const BeamArgs&, const int32_t* entry, int cnt, int, const FrameScratch&)
    {
        const int CK = a.m.K;
        const uint8_t* wn = win.nxt;
        for (int i = threadIdx.x; i < cnt * CK; i += NT) {
            const int e = i / CK, s = i - e * CK;
            tile_ids[i] = wn[(size_t)entry[e] * WIN + s];
        }
        __syncthreads();
        nnlm_tile(a.m, tile_ids, cnt, tile_act, tile_rows);
    }
    __device__ __forceinline__ void flip()
    {
        rows.flip();
        win.flip();
    }
    __device__ __forceinline__ void new_rows(const BeamArgs& p, const Beam& NB, int nsel, int t, const FrameScratch& f)
    {
        neural_rows(*this, p, NB, nsel, t, f);
    }
};

struct RNNArgs {
    RNNLMDev m;
    int32_t state_copies;   // 1; SCTC_RNNBEAM_STATE_COPIES = 2..4 repeats the copy of the carried states, which
                            // changes no result: the time it adds is what the copy costs (tools/decode_rnn_bench.py)
};

// every beam entry carries the LM's hidden state of its prefix: copied from its parent when carried
// over, one recurrent step from the parent's state and the new symbol when new
struct RNNPolicy : NeuralRows {
    using Args = RNNArgs;
    const Args& a;
    BeamPair<float> st;   // the hidden states, [K][H]
    int32_t* tile_slot;   // LM id, parent's state row and own state row of every slot of one tile

    __device__ __forceinline__ RNNPolicy(const BeamArgs&, const Args& args) : a(args) {}
    __device__ __forceinline__ char* carve(char* w, const BeamArgs& p)
    {
        w = carve_rows(w, p);
        const int H = a.m.H;
        st.carve(w, (size_t)p.K * H);
        w += align256((size_t)2 * p.K * H * sizeof(float));
        tile_act = (float*)w;
        tile_rows = (float*)(w + nn_act_bytes(H));
        tile_slot = (int32_t*)(w + nn_act_bytes(H) + nn_row_bytes(a.m.Vp));
        return w + rnn_tile_bytes(H, a.m.Vp);
    }
    // the empty prefix: <s> into the zero state
    __device__ __forceinline__ void empty_rows(const BeamArgs& p, const Beam&)
    {
        if (threadIdx.x == 0) {
            tile_slot[0] = a.m.bos;
            tile_slot[NN_TILE] = 0;
            tile_slot[2 * NN_TILE] = 0;
        }
        __syncthreads();
        rnnlm_tile(a.m, tile_slot, 1, nullptr, st.cur, tile_act, tile_rows);
        first_row(p);
    }
    __device__ __forceinline__ void carry(const BeamArgs&, const Beam&, Beam&, const State&, State&, int, int) {}
    __device__ __forceinline__ void extend(const BeamArgs&, const Beam&, Beam&, const State&, State&, int, int, int) {}
    // a carried entry keeps its state: a copy into the new beam's buffer, by the whole workgroup
    __device__ __forceinline__ void carry_shared(const Beam& NB, int nsel)
    {
        const int Hq = a.m.H >> 2;
        const float4* so = (const float4*)st.cur;
        float4* sn = (float4*)st.nxt;
        for (int pass = 0; pass < a.state_copies; ++pass)
            for (int it = threadIdx.x; it < nsel * Hq; it += NT) {
                const int r = it / Hq;
                const int src = NB.prev[r];
                if (src >= 0) sn[it] = so[(size_t)src * Hq + (it - r * Hq)];
            }
    }
    // the parent j and the symbol c as step 3 recorded them: the parent's state is in the old beam's
    // buffer, the entry's goes to the new one
    __device__ __forceinline__ void run_tile(const BeamArgs& p, const int32_t* entry, int cnt, int t, const FrameScratch& f)
    {
        const int tid = threadIdx.x;
        if (tid < cnt) {
            const int r = entry[tid];
            const int ev = f.rec[(int64_t)t * p.K + r];
            tile_slot[tid] = p.sym_word[ev & 0xFFFF];
            tile_slot[NN_TILE + tid] = ev >> 16;
            tile_slot[2 * NN_TILE + tid] = r;
        }
        __syncthreads();
        rnnlm_tile(a.m, tile_slot, cnt, st.cur, st.nxt, tile_act, tile_rows);
    }
    __device__ __forceinline__ void flip()
    {
        rows.flip();
        st.flip();
    }
    __device__ __forceinline__ void new_rows(const BeamArgs& p, const Beam& NB, int nsel, int t, const FrameScratch& f)
    {
        neural_rows(*this, p, NB, nsel, t, f);
    }
};

}  // namespace beam
}  // namespace sctc
