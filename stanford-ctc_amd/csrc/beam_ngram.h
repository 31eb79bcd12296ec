// The prefix beam search with a character n-gram LM, or with none: ctc_beam_kernel's
// body.  It is the search of beam_search.h written out for this one LM, statement for statement the
// code the kernel had before the other three searches moved behind policies, and it stays apart from
// them for one reason: through beam_search<Policy> the same statements compiled to a kernel that was
// 0.4 - 0.9 % slower (profiles/decode_refactor.md), and this is the most used of the four.  The types
// and helpers are beam_search.h's; a change to the frame loop, the select or the ranks is made in
// both files.
#pragma once
#include "beam_search.h"

namespace sctc {
namespace beam {

// the kernel's one argument; the order is the one the kernel was measured with
struct NgramBeamArgs {
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
};

__device__ inline uint64_t bytes_mask(int m) { return m >= 8 ? ~0ull : ((1ull << (8 * m)) - 1); }

__device__ inline bool lm_find(const NgramBeamArgs& p, uint64_t key, float& pr, float& bo)
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
__device__ float lm_score(const NgramBeamArgs& p, uint64_t ctx, int ctxlen, uint32_t w)
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

__device__ __forceinline__ void ngram_beam_search(const NgramBeamArgs& p)
{
    __shared__ Beam bm[2];
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
    const bool has_lm = p.lm_key != nullptr;
    const int ctx_max = has_lm ? p.lm_order - 1 : 0;
    const uint64_t ctx_mask = bytes_mask(ctx_max);

    char* w = p.ws + u.ws_off;
    float2* cand[2] = {(float2*)w, (float2*)w + M};
    w += align256(2 * M * sizeof(float2));
    uint64_t* ckey = (uint64_t*)w;
    w += align256(M * sizeof(uint64_t));
    float* rows[2] = {(float*)w, (float*)w + M};
    if (has_lm) w += align256(2 * M * sizeof(float));
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
    }
    __syncthreads();
    if (tid == 0) htab_insert(tab[0], H_EMPTY_PREFIX, 0);
    if (has_lm)
        for (int c = tid; c < A; c += NT)
            rows[0][c] = c == 0 ? 0.0f : lm_score(p, bm[0].ctx[0], ctx_max < 1 ? ctx_max : 1, (uint32_t)p.sym_word[c]);
    __syncthreads();

    int n = 1, cb = 0, tc = 0, rb = 0;
    for (int t = 0; t < T; ++t) {
        const Beam& B = bm[cb];
        Beam& NB = bm[cb ^ 1];
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
                        const double lmp = has_lm ? p.alpha * (double)rows[rb][pj * A + l] : 0.0;
                        const double e1 = (double)B.pb[pj] + y[l] + lmp;
                        const double e0 = B.last[pj] != l ? (double)B.pnb[pj] + y[l] + lmp : -INFINITY;
                        nb = lse3(t0, e0, e1);
                    } else {
                        nb = t0;
                    }
                }
                bb = lse2(v0 + y0, v1 + y0);
                klen = B.len[j];
            } else {
                const uint64_t H = hstep(B.h[j], c);
                if (htab_find(cur, H) >= 0) {          // P+c is a beam entry: counted there
                    ckey[idx] = 0;
                    cand[cw][idx] = make_float2(-INFINITY, -INFINITY);
                    continue;
                }
                const double lmw = has_lm ? p.alpha * (double)rows[rb][idx] : 0.0;
                const double e1 = v1 + y[c] + lmw;
                const double e0 = c != l ? v0 + y[c] + lmw : -INFINITY;
                float2 hv = make_float2(-INFINITY, -INFINITY);
                const int q = htab_find(old, H);
                if (q >= 0) hv = cand[cr][(int64_t)q * A];
                else if (B.prev[j] >= 0) hv = cand[cr][(int64_t)B.prev[j] * A + c];
                nb = lse3(e0, e1, (double)hv.x + y[c]);
                bb = lse2((double)hv.x + y0, (double)hv.y + y0);
                klen = B.len[j] + 1;
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
            } else {
                NB.h[r] = hstep(B.h[j], c);
                NB.ph[r] = B.h[j];
                NB.ctx[r] = has_lm ? (((B.ctx[j] << 8) | (uint64_t)p.sym_word[c]) & ctx_mask) : 0;
                NB.last[r] = c;
                NB.len[r] = B.len[j] + 1;
                NB.prev[r] = -1;
            }
            rec[(int64_t)t * K + r] = (j << 16) | c;
        }
        // the previous beam's table is no longer needed: it becomes the new beam's
        HTab& nt = tab[tc ^ 1];
        for (int s = tid; s < HT; s += NT) nt.idx[s] = -1;
        __syncthreads();
        if (tid < nsel) htab_insert(nt, NB.h[tid], tid);

        // ---- 4. LM rows: carried entries keep theirs, new ones query the LM ----------------
        if (has_lm) {
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

}  // namespace beam
}  // namespace sctc
