// The body of the CTC prefix beam search: the reference's BeamLMDecoder.decode
// (ctc_fast/new_decoder/decoder.pyx:136-193) for one utterance per workgroup, every frame of the
// search inside one launch.  Per frame:
//   1. cells: beam entry j (rank order) and symbol c form cell j*A + c -- c == 0 is the
//      prefix itself (blank and repeat terms, plus its parent's extension when the parent is
//      in the beam), c >= 1 the extension P+c (LM term, plus the "Hold" masses of P+c among
//      the previous frame's candidates); an extension that IS a beam entry is disabled (its
//      mass arrives through that entry's own cell), so every prefix is counted once;
//   2. top-`beam` select: radix select over order-preserving 64-bit keys of the float64
//      sort key, ties by ascending cell index; then ranks by counting;
//   3. the new beam: float32 masses, 64-bit prefix hashes, a back-pointer per entry and frame
//      (the hypotheses are read back through them at the end);
//   4. what the LM keeps per entry (its rows, log10 P(c | prefix) for all c) for the new beam.
//
// Frame loop, cell arithmetic, select, ranks, hash tables, back-pointers and the n-best read-back are
// written here for the lexicon and the two neural searches (the n-gram search: beam_ngram.h).  Everything that depends on the LM goes through the hooks of a policy
// (beam_policies.h has the three); a hook is a __forceinline__ member, so a kernel holds the code
// of its own policy and nothing of the others:
//
//   Policy(p, args)                       from the kernel's arguments
//   carve(w, p)                           its part of the workspace slice, between the keys and the back-pointers
//   empty_entry(p, b0, x0)                the empty prefix: its per-entry state (thread 0)
//   empty_rows(p, b0)                     the empty prefix: its rows (every thread; may hold barriers)
//   candidate(p, X, j, c)                 may symbol c >= 1 extend entry j at all
//   lm_term(p, X, e, c)                   the LM term of entry e extended by c (also the parent-extension term of cell c == 0)
//   counted_len(p, B, X, j, c)            the length the bonus counts: of entry j (c == 0) or of its extension by c
//   carry(p, B, NB, X, NX, j, r)          what entry r copies from entry j it carries over
//   extend(p, B, NB, X, NX, j, c, r)      what entry r computes as j extended by c
//   new_rows(p, NB, nsel, t, f)           step 4 (every thread; may hold barriers, under conditions uniform
//                                         over the workgroup); flips the policy's own buffers to the new beam
//   Policy::State                         per-entry LDS state of a beam (an empty struct for none)
#pragma once
#include <math.h>

#include "beam_limits.h"
#include "common.h"

namespace sctc {
namespace beam {

constexpr int NT = 256;       // threads per workgroup
constexpr int HT = 512;       // slots of a beam hash table (load <= 1/2)
constexpr uint64_t H_EMPTY_PREFIX = 0x6A09E667F3BCC909ull;

struct UttDesc {
    int64_t frame_off;   // first row of the utterance in probs
    int64_t ws_off;      // byte offset of its workspace slice
    int64_t id_off;      // first hypothesis element: ids[nbest * id_off + n * T + i]
    int32_t T;
    int32_t pad;
};

// What every search reads; a policy's own arguments are a second kernel argument.  The order is part of the
// kernels' speed: the compiler fetches the arguments in blocks of 8 and 16 dwords and spills a block as a
// whole, so what a workgroup reads once (the first 32 bytes, and `scores`) stays apart from what its loops
// read.  The three kernels were measured with this order; with the two kinds mixed in one block the lexicon
// kernel reloads spilled scalars in 259 places, with this order in 118 (profiles/decode_refactor.md).
struct BeamArgs {
    const UttDesc* utt;
    char* ws;
    int32_t* ids;
    int32_t* lens;
    double* scores;
    const void* probs;
    int64_t ld;
    int32_t f64;
    int32_t A, K, nbest;
    double alpha, beta;
    const int32_t* sym_word;   // device [A]: the LM's id of every symbol (zeros for a search without a map)
};
static_assert(offsetof(BeamArgs, scores) == 32 && offsetof(BeamArgs, probs) == 40 && offsetof(BeamArgs, sym_word) == 88 &&
                  sizeof(BeamArgs) == 96,
              "BeamArgs: read-once fields first; measure the three searches before changing the order");

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

struct Beam {
    uint64_t h[KMAX];     // prefix hash
    uint64_t ph[KMAX];    // hash of the prefix without its last symbol
    uint64_t ctx[KMAX];   // the n-gram search's LM context: last (order-1) word ids of <s> + P
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

template <typename Args>
__device__ inline double load_prob(const Args& p, int64_t row, int c)
{
    return p.f64 ? ((const double*)p.probs)[row * p.ld + c] : (double)((const float*)p.probs)[row * p.ld + c];
}

// what step 4 of a policy may use of the frame: the back-pointers step 3 wrote, and two LDS arrays
// that are free until the next select
struct FrameScratch {
    const int32_t* rec;   // rec[t * K + r] = (j << 16) | c of entry r of frame t
    int32_t* sel_idx;     // [KMAX]
    int32_t* scan;        // block_excl_scan's scratch
};

template <typename Policy>
__device__ __forceinline__ void beam_search(const BeamArgs& p, const typename Policy::Args& pa)
{
    using State = typename Policy::State;
    __shared__ Beam bm[2];
    __shared__ State lx[2];
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
    Policy pol(p, pa);

    char* w = p.ws + u.ws_off;
    float2* cand[2] = {(float2*)w, (float2*)w + M};
    w += align256(2 * M * sizeof(float2));
    uint64_t* ckey = (uint64_t*)w;
    w += align256(M * sizeof(uint64_t));
    w = pol.carve(w, p);
    int32_t* rec = (int32_t*)w;

    for (int s = tid; s < HT; s += NT) {
        tab[0].idx[s] = -1;
        tab[1].idx[s] = -1;
    }
    if (tid == 0) {
        bm[0].h[0] = H_EMPTY_PREFIX;
        bm[0].ph[0] = 0;
        bm[0].key[0] = 0.0;
        bm[0].pnb[0] = -INFINITY;
        bm[0].pb[0] = 0.0f;
        bm[0].last[0] = -1;
        bm[0].len[0] = 0;
        bm[0].prev[0] = -1;
        pol.empty_entry(p, bm[0], lx[0]);
    }
    __syncthreads();
    if (tid == 0) htab_insert(tab[0], H_EMPTY_PREFIX, 0);
    pol.empty_rows(p, bm[0]);
    __syncthreads();

    int n = 1, cb = 0, tc = 0;
    for (int t = 0; t < T; ++t) {
        const Beam& B = bm[cb];
        Beam& NB = bm[cb ^ 1];
        const State& X = lx[cb];
        State& NX = lx[cb ^ 1];
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
                        const double lmp = pol.lm_term(p, X, pj, l);
                        const double e1 = (double)B.pb[pj] + y[l] + lmp;
                        const double e0 = B.last[pj] != l ? (double)B.pnb[pj] + y[l] + lmp : -INFINITY;
                        nb = lse3(t0, e0, e1);
                    } else {
                        nb = t0;
                    }
                }
                bb = lse2(v0 + y0, v1 + y0);
                klen = pol.counted_len(p, B, X, j, 0);
            } else {
                const uint64_t H = hstep(B.h[j], c);
                // no candidate, or P+c is a beam entry and counted there
                if (!pol.candidate(p, X, j, c) || htab_find(cur, H) >= 0) {
                    ckey[idx] = 0;
                    cand[cw][idx] = make_float2(-INFINITY, -INFINITY);
                    continue;
                }
                const double lmw = pol.lm_term(p, X, j, c);
                const double e1 = v1 + y[c] + lmw;
                const double e0 = c != l ? v0 + y[c] + lmw : -INFINITY;
                float2 hv = make_float2(-INFINITY, -INFINITY);
                const int q = htab_find(old, H);
                if (q >= 0) hv = cand[cr][(int64_t)q * A];
                else if (B.prev[j] >= 0) hv = cand[cr][(int64_t)B.prev[j] * A + c];
                nb = lse3(e0, e1, (double)hv.x + y[c]);
                bb = lse2((double)hv.x + y0, (double)hv.y + y0);
                klen = pol.counted_len(p, B, X, j, c);
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
                NB.last[r] = B.last[j];
                NB.len[r] = B.len[j];
                NB.prev[r] = j;
                pol.carry(p, B, NB, X, NX, j, r);
            } else {
                NB.h[r] = hstep(B.h[j], c);
                NB.ph[r] = B.h[j];
                NB.last[r] = c;
                NB.len[r] = B.len[j] + 1;
                NB.prev[r] = -1;
                pol.extend(p, B, NB, X, NX, j, c, r);
            }
            rec[(int64_t)t * K + r] = (j << 16) | c;
        }
        // the previous beam's table is no longer needed: it becomes the new beam's
        HTab& nt = tab[tc ^ 1];
        for (int s = tid; s < HT; s += NT) nt.idx[s] = -1;
        __syncthreads();
        if (tid < nsel) htab_insert(nt, NB.h[tid], tid);

        // ---- 4. LM rows: carried entries keep theirs, new ones query the LM ----------------
        pol.new_rows(p, NB, nsel, t, FrameScratch{rec, sel_idx, scan_scratch});
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
