// Minimum Bayes risk selection over n-best lists, word interning and word confidences on the device.
//
//   interning   sctc_intern_words_batch gives every token of a group of label rows an id, so that two tokens have the
//               same id exactly when they are the same run of symbols: the id of token t is the smallest t' <= t (in
//               (row, position) order) with the same symbols.  Four launches: tokens (a wave per row: the ballots of
//               word_lm_score_kernel give the token starts, the lane at a start walks the token for its length and
//               hash), the tokens of the earlier rows of the group (a wave per group), insertion into the group's hash
//               table (a lane per token; a compare-and-swap claims an empty entry, an entry that holds the same
//               symbols -- always compared, a hash alone decides nothing -- takes atomicMin of the token's slot) and
//               the read of the representative.  Which entry a word ends up in depends on who came first; the value
//               left in it, the smallest slot of the word, does not: the ids are the same bits from run to run.
//   distances   nbest_dist_kernel: one wave per unordered pair (k < j) of real hypotheses of an utterance, edit_pair
//               of edit_dev.h on the symbols or the word ids; the wave finds its utterance by bisection over the B
//               first-pair numbers and its pair by walking the rows of the triangle.  No descriptor per pair.
//   choice      nbest_mbr_kernel: one wave per utterance, float64, no contraction, no atomics; the sums run in
//               ascending rank in every lane.
//   confidences nbest_conf_kernel: one wave per (utterance, hypothesis j) aligns the chosen hypothesis with j
//               (edit_pair<true>) and marks the units of the chosen one that the path matches;
//               nbest_conf_sum_kernel: one wave per utterance adds the weights of the hypotheses that agree.
#include <math.h>

#include <cmath>
#include <vector>

#include "common.h"
#include "edit_dev.h"
#include "nbest_mbr_plan.h"

namespace sctc {
namespace {

constexpr uint32_t INTERN_EMPTY = 0xffffffffu;

struct InternArgs {
    const InternRow* rows;      // workspace
    const InternGroup* groups;  // workspace
    int32_t* base;              // workspace [N]
    InternMeta* meta;           // workspace [slots]
    uint32_t* table;            // workspace
    const int32_t* labels;
    int32_t* word_ids;
    int32_t* counts;
    int32_t* status;
    int64_t n_slots;
    int32_t N, G, A, space;
};

// a wave per row: status, count, and where every token lies
__global__ __launch_bounds__(256) void intern_words_kernel(InternArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= p.N) return;       // whole waves leave; there is no workgroup barrier below
    const InternRow d = p.rows[n];
    const int32_t* l = p.labels + d.label_off;
    const int U = d.U, A = p.A, space = p.space;
    const unsigned long long below = (1ull << lane) - 1;
    bool bad = false;
    for (int base = 0; base < U; base += 64) {
        const int i = base + lane;
        const int c = l[min(i, U - 1)];
        bad |= i < U && (c < 1 || c >= A);
    }
    const bool any_bad = __any(bad) != 0;
    int starts = 0;
    bool carry_sp = true;       // the symbol before the chunk is a space (or the row's start)
    for (int base = 0; base < U && !any_bad; base += 64) {
        const int i = base + lane;
        const bool in = i < U;
        const int c = l[min(i, U - 1)];
        const bool sp = !in || c == space;
        const unsigned long long spm = __ballot(sp);
        const bool after_sp = lane == 0 ? carry_sp : ((spm >> (lane - 1)) & 1) != 0;
        const bool start = !sp && after_sp;
        const unsigned long long stm = __ballot(start);
        if (start) {
            uint32_t h = 2166136261u;       // FNV-1a over the symbols; only ever a hint, the symbols decide
            int j = i, cj = c;
            while (true) {
                h = (h ^ (uint32_t)cj) * 16777619u;
                if (++j >= U) break;
                cj = l[j];
                if (cj == space) break;
            }
            InternMeta m;
            m.off = d.label_off + i;
            m.len = j - i;
            m.hash = h;
            m.row = (int32_t)n;
            m.pad = 0;
            p.meta[d.slot_off + starts + __popcll(stm & below)] = m;
        }
        starts += __popcll(stm);
        carry_sp = (spm >> 63) != 0;
    }
    if (lane == 0) {
        p.counts[n] = starts;
        p.status[n] = any_bad ? 2 : 0;
    }
}

// a wave per group: base[r] = tokens of the group's rows before r
__global__ __launch_bounds__(256) void intern_base_kernel(InternArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= p.G) return;
    const InternGroup grp = p.groups[g];
    int run = 0;
    for (int r0 = grp.first; r0 < grp.end; r0 += 64) {
        const int r = r0 + lane;
        const int v = p.counts[min(r, grp.end - 1)];
        const int c = r < grp.end ? v : 0;
        int ex = 0, tot = 0;
        for (int j = 0; j < 64; ++j) {
            const int cj = rdlane(c, j);
            ex += j < lane ? cj : 0;
            tot += cj;
        }
        if (r < grp.end) p.base[r] = run + ex;
        run += tot;
    }
}

__device__ __forceinline__ bool same_word(const int32_t* labels, const InternMeta& x, int64_t y_off, int32_t y_len, uint32_t y_hash)
{
    if (x.len != y_len || x.hash != y_hash) return false;
    for (int i = 0; i < y_len; ++i)
        if (labels[x.off + i] != labels[y_off + i]) return false;
    return true;
}

// a lane per word slot: the token's word goes into the group's table, or finds itself there; the entry keeps the
// smallest slot of the word.  The entry's index waits in word_ids for intern_resolve_kernel.
__global__ __launch_bounds__(256) void intern_insert_kernel(InternArgs p)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n_slots) return;
    const InternMeta m = p.meta[s];
    if (m.len < 0) return;
    const InternRow d = p.rows[m.row];
    uint32_t* tab = p.table + d.tab_off;
    uint32_t pos = m.hash & d.tab_mask;
    while (true) {
        const uint32_t cur = atomicCAS(&tab[pos], INTERN_EMPTY, (uint32_t)s);
        if (cur == INTERN_EMPTY) break;
        // whichever token of a word sits in the entry, its symbols are the word's
        if (same_word(p.labels, p.meta[cur], m.off, m.len, m.hash)) {
            atomicMin(&tab[pos], (uint32_t)s);
            break;
        }
        pos = (pos + 1) & d.tab_mask;
    }
    p.word_ids[s] = (int32_t)pos;
}

// a lane per word slot: the id is the token number, within the group, of the word's first token
__global__ __launch_bounds__(256) void intern_resolve_kernel(InternArgs p)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n_slots) return;
    const InternMeta m = p.meta[s];
    if (m.len < 0) return;
    const InternRow d = p.rows[m.row];
    const uint32_t rep = p.table[d.tab_off + (uint32_t)p.word_ids[s]];
    const int rrow = p.meta[rep].row;
    p.word_ids[s] = p.base[rrow] + (int32_t)((int64_t)rep - p.rows[rrow].slot_off);
}

struct MbrArgs {
    const int64_t* row_off;     // workspace [B * K]
    const MbrUtt* utts;         // workspace: the launch's utterances
    const int32_t* kb;          // workspace [B]
    const int32_t* lens;        // workspace [B * K]
    const int32_t* units;       // the labels, or the word ids
    const double* scores;
    const int32_t* order;       // or nullptr
    int32_t* dist;
    double* post;
    double* risk;
    int32_t* best;
    int32_t* mbr_order;
    double* w;                  // workspace, with confidences only (else nullptr)
    double* z;
    int8_t* match;
    int8_t* ops;
    char* tab;
    double* conf;
    int32_t* conf_len;
    size_t tab_stride;
    int64_t n_pairs;
    double scale;
    int32_t B, K, n_utts, slot;
};

__device__ __forceinline__ bool mbr_real(const MbrArgs& p, int64_t b, int k, int kb)
{
    const double s = p.scores[b * p.K + min(k, p.K - 1)];
    return k < kb && isfinite(s);
}

// a lane per entry of D: the diagonal, and everything of a rank that is not real
__global__ __launch_bounds__(256) void nbest_fill_kernel(MbrArgs p)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t KK = (int64_t)p.K * p.K;
    if (idx >= p.B * KK) return;
    const int64_t b = idx / KK;
    const int k = (int)((idx - b * KK) / p.K), j = (int)(idx - b * KK - (int64_t)k * p.K);
    const int kb = p.kb[b];
    const bool both = mbr_real(p, b, k, kb) && mbr_real(p, b, j, kb);
    if (!both) p.dist[idx] = -1;
    else if (k == j) p.dist[idx] = 0;
}

__global__ __launch_bounds__(64 * WAVES) void nbest_dist_kernel(MbrArgs p)
{
    extern __shared__ __align__(16) char mbr_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= p.n_pairs) return;       // whole waves leave; there is no barrier below
    // the last utterance whose first pair is not beyond idx has the pair (one without pairs shares its number with
    // the next)
    int lo = 0, hi = p.n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.utts[mid].pair_off <= idx) lo = mid;
        else hi = mid - 1;
    }
    const MbrUtt u = p.utts[lo];
    const int kb = u.kb;
    int k = 0, rem = (int)(idx - u.pair_off);
    while (rem >= kb - 1 - k) {
        rem -= kb - 1 - k;
        ++k;
    }
    const int j = k + 1 + rem;
    const int64_t b = u.b;
    if (!(mbr_real(p, b, k, kb) && mbr_real(p, b, j, kb))) return;     // nbest_fill_kernel wrote the -1
    char* slot = mbr_lds + (size_t)wave * p.slot;
    EditPair d{};
    d.a_off = p.row_off[b * p.K + k];
    d.b_off = p.row_off[b * p.K + j];
    d.n = __builtin_amdgcn_readfirstlane(p.lens[b * p.K + k]);
    d.m = __builtin_amdgcn_readfirstlane(p.lens[b * p.K + j]);
    EditArgs e{};
    e.a = p.units;
    e.b = p.units;
    e.stats = (int32_t*)slot;
    edit_pair<false>(e, d, slot + MBR_STAT_BYTES, lane);
    if (lane == 0) {            // the lane that wrote the counts
        const int dist = ((const int32_t*)slot)[0];
        p.dist[(b * p.K + k) * p.K + j] = dist;
        p.dist[(b * p.K + j) * p.K + k] = dist;
    }
}

__device__ __forceinline__ void wave_sync_lds()
{
    // every lane reads what every lane of this wave wrote
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(256) void nbest_mbr_kernel(MbrArgs p)
{
#pragma clang fp contract(off)
    __shared__ double s_w[4][MBR_MAX_K], s_r[4][MBR_MAX_K];
    __shared__ int s_pos[4][MBR_MAX_K], s_real[4][MBR_MAX_K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= p.B) return;       // whole waves leave; there is no workgroup barrier below
    const int K = p.K, kb = p.kb[b];
    double* w = s_w[wave];
    double* rk = s_r[wave];
    int* pos = s_pos[wave];
    int* real = s_real[wave];
    double mx = -INFINITY;
    int n_real = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const double s = p.scores[b * K + min(k, K - 1)];
        const bool r = k < kb && isfinite(s);
        mx = r && s > mx ? s : mx;
        n_real += __popcll(__ballot(r));
        if (k < K) {
            real[k] = r;
            pos[k] = k;
        }
    }
    mx = wave_max(mx);
    wave_sync_lds();
    if (p.order)
        for (int i = lane; i < K; i += 64) {
            const int o = p.order[b * K + i];
            if (o >= 0 && o < K) pos[o] = i;
        }
    for (int k = lane; k < K; k += 64) {
        const double s = p.scores[b * K + k];
        const double e = exp(p.scale * (s - mx));
        w[k] = real[k] ? (s == mx ? 1.0 : e) : 0.0;     // exactly 1.0 at the maximum, whatever exp(0) gives
    }
    wave_sync_lds();
    double Z = 0.0;
    for (int k = 0; k < K; ++k) Z += w[k];              // ascending; a rank that is not real adds +0.0
    for (int k = lane; k < K; k += 64) {
        double acc = 0.0;
        for (int j = 0; j < K; ++j) {
            const double t = w[j] * (double)p.dist[(b * K + j) * K + k];       // D is symmetric: row j, my column
            acc += real[j] ? t : 0.0;
        }
        const double r = real[k] ? acc / Z : INFINITY;
        rk[k] = r;
        p.risk[b * K + k] = r;
        p.post[b * K + k] = real[k] ? w[k] / Z : 0.0;
        if (p.w) p.w[b * K + k] = w[k];
    }
    wave_sync_lds();
    for (int k = lane; k < K; k += 64) {
        int r = 0;
        if (real[k]) {
            const double v = rk[k];
            const int pk = pos[k];
            for (int j = 0; j < K; ++j) {
                const double vj = rk[j];
                const int pj = pos[j];
                const bool first = vj < v || (vj == v && (pj < pk || (pj == pk && j < k)));
                r += real[j] && first;
            }
            if (r == 0) p.best[b] = k;
        } else {                // the ranks that are not real come last, in their original order
            r = n_real;
            for (int j = 0; j < k; ++j) r += !real[j];
        }
        p.mbr_order[b * K + r] = k;
    }
    if (lane == 0) {
        if (n_real == 0) p.best[b] = -1;
        if (p.z) p.z[b] = Z;
    }
}

// one wave per (utterance of the launch, hypothesis j): which units of the chosen hypothesis does j agree with
__global__ __launch_bounds__(64 * WAVES) void nbest_conf_kernel(MbrArgs p)
{
    extern __shared__ __align__(16) char mbr_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= (int64_t)p.n_utts * p.K) return;     // whole waves leave; there is no workgroup barrier below
    const MbrUtt u = p.utts[idx / p.K];
    const int j = (int)(idx % p.K);
    const int64_t b = u.b;
    const int c = __builtin_amdgcn_readfirstlane(p.best[b]);
    if (c < 0 || j == c || !mbr_real(p, b, j, u.kb)) return;
    char* slot = mbr_lds + (size_t)wave * p.slot;
    int32_t* st = (int32_t*)slot;
    EditPair d{};
    d.a_off = p.row_off[b * p.K + c];
    d.b_off = p.row_off[b * p.K + j];
    d.n = __builtin_amdgcn_readfirstlane(p.lens[b * p.K + c]);
    d.m = __builtin_amdgcn_readfirstlane(p.lens[b * p.K + j]);
    const int64_t first = (int64_t)p.K * u.conf_off + (int64_t)j * u.longest;
    d.ops_off = 2 * first;
    const size_t edge_b = d.n > 0 && d.m > PANEL ? (size_t)d.n * sizeof(int2) : 0;
    const size_t tab_b = d.n > 0 && d.m > 0 ? (size_t)((d.n + 3) / 4) * ((d.m + CPL - 1) / CPL) * sizeof(uint32_t) : 0;
    d.lds_tab = MBR_STAT_BYTES + edge_b + tab_b <= (size_t)p.slot;
    d.tab_off = (int64_t)((b * p.K + j) * (int64_t)p.tab_stride);
    EditArgs e{};
    e.a = p.units;
    e.b = p.units;
    e.stats = st;
    e.ops = p.ops;
    e.ops_len = st + 5;
    e.ws = p.tab;
    edit_pair<true>(e, d, slot + MBR_STAT_BYTES, lane);
    wave_sync_lds();            // without a table (an empty side) every lane wrote a part of the path
    if (lane == 0) {
        const int len = st[5];
        const int8_t* ops = p.ops + d.ops_off;
        int8_t* mt = p.match + first;
        int i = 0;
        for (int q = 0; q < len && i < d.n; ++q) {
            const int op = ops[q];
            if (op != OP_LEFT) mt[i++] = op == OP_MATCH;
        }
    }
}

// one wave per utterance of the launch: conf[i] = (sum over the real ranks j, ascending, of w_j * match_j[i]) / Z
__global__ __launch_bounds__(256) void nbest_conf_sum_kernel(MbrArgs p)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t ui = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ui >= p.n_utts) return;
    const MbrUtt u = p.utts[ui];
    const int64_t b = u.b;
    const int K = p.K;
    const int c = p.best[b];
    const int n = p.lens[b * K + max(c, 0)];
    const int len = c >= 0 ? n : 0;
    if (lane == 0) p.conf_len[b] = len;
    const double Z = p.z[b];
    for (int i = lane; i < len; i += 64) {
        double acc = 0.0;
        for (int j = 0; j < K; ++j) {
            const int mj = p.match[(int64_t)K * u.conf_off + (int64_t)j * u.longest + i];
            const double t = p.w[b * K + j] * (double)(j == c ? 1 : mj);
            acc += mbr_real(p, b, j, u.kb) ? t : 0.0;
        }
        p.conf[u.conf_off + i] = acc / Z;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------

int check_intern(const sctc_intern_config* cfg)
{
    SCTC_CHECK_ARG(cfg, "intern_words: null config");
    SCTC_CHECK_ARG(cfg->N >= 0 && cfg->G >= 0, "intern_words: %d rows, %d groups", cfg->N, cfg->G);
    SCTC_CHECK_ARG(cfg->A >= 1 && cfg->A <= 256, "intern_words: alphabet of %d symbols outside 1..256", cfg->A);
    SCTC_CHECK_ARG(cfg->space >= 1 && cfg->space < cfg->A, "intern_words: space %d outside [1, %d)", cfg->space, cfg->A);
    SCTC_CHECK_ARG(cfg->group_off, "intern_words: null group_off");
    SCTC_CHECK_ARG(cfg->N == 0 || (cfg->U_b && cfg->label_off), "intern_words: null length / offset array");
    SCTC_CHECK_ARG(cfg->group_off[0] == 0 && cfg->group_off[cfg->G] == cfg->N,
                   "intern_words: group_off runs from %d to %d, not from 0 to %d", cfg->group_off[0], cfg->group_off[cfg->G], cfg->N);
    for (int g = 0; g < cfg->G; ++g)
        SCTC_CHECK_ARG(cfg->group_off[g] <= cfg->group_off[g + 1], "intern_words: group_off decreases at group %d", g);
    int64_t slots = 0;
    for (int n = 0; n < cfg->N; ++n) {
        SCTC_CHECK_ARG(cfg->U_b[n] >= 0 && cfg->U_b[n] <= MBR_MAX_U, "intern_words: row %d has %d labels, outside 0..%d", n,
                       cfg->U_b[n], MBR_MAX_U);
        SCTC_CHECK_ARG(cfg->label_off[n] >= 0, "intern_words: row %d has a negative offset", n);
        slots += intern_row_slots(cfg->U_b[n]);
    }
    SCTC_CHECK_ARG(slots < (1ll << 31), "intern_words: %lld word slots, the limit is 2^31 - 1", (long long)slots);
    return SCTC_OK;
}

// the four launches; `ws` holds the uploaded descriptors at the plan's offsets
int launch_intern(const InternPlan& pl, int32_t N, int32_t G, int32_t A, int32_t space, const int32_t* labels_dev,
                  int32_t* word_ids_dev, int32_t* counts_dev, int32_t* status_dev, char* ws, hipStream_t s)
{
    InternArgs a{};
    a.rows = (const InternRow*)(ws + pl.off_rows);
    a.groups = (const InternGroup*)(ws + pl.off_groups);
    a.base = (int32_t*)(ws + pl.off_base);
    a.meta = (InternMeta*)(ws + pl.off_meta);
    a.table = (uint32_t*)(ws + pl.off_table);
    a.labels = labels_dev;
    a.word_ids = word_ids_dev;
    a.counts = counts_dev;
    a.status = status_dev;
    a.n_slots = pl.n_slots;
    a.N = N;
    a.G = G;
    a.A = A;
    a.space = space;
    if (pl.fill_bytes) SCTC_HIP_TRY(hipMemsetAsync(ws + pl.off_meta, 0xff, pl.fill_bytes, s));
    hipLaunchKernelGGL(intern_words_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    if (pl.n_slots == 0) return SCTC_OK;
    const dim3 per_slot((unsigned)((pl.n_slots + 255) / 256));
    hipLaunchKernelGGL(intern_base_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(intern_insert_kernel, per_slot, dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(intern_resolve_kernel, per_slot, dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

void intern_head(const InternPlan& pl, char* image)
{
    if (!pl.rows.empty()) memcpy(image + pl.off_rows, pl.rows.data(), pl.rows.size() * sizeof(InternRow));
    if (!pl.groups.empty()) memcpy(image + pl.off_groups, pl.groups.data(), pl.groups.size() * sizeof(InternGroup));
}

constexpr int MBR_KNOWN_FLAGS = SCTC_MBR_CONF | SCTC_MBR_DIST;

int check_mbr(const sctc_mbr_config* cfg)
{
    SCTC_CHECK_ARG(cfg, "nbest_mbr: null config");
    SCTC_CHECK_ARG(cfg->B >= 0, "nbest_mbr: %d utterances", cfg->B);
    SCTC_CHECK_ARG(cfg->K >= 1 && cfg->K <= MBR_MAX_K, "nbest_mbr: %d hypotheses outside 1..%d", cfg->K, MBR_MAX_K);
    SCTC_CHECK_ARG(cfg->unit == SCTC_MBR_CHARS || cfg->unit == SCTC_MBR_WORDS, "nbest_mbr: unknown unit %d", cfg->unit);
    SCTC_CHECK_ARG((cfg->flags & ~MBR_KNOWN_FLAGS) == 0, "nbest_mbr: unknown flags 0x%x", cfg->flags);
    SCTC_CHECK_ARG(cfg->A >= 1 && cfg->A <= 256, "nbest_mbr: alphabet of %d symbols outside 1..256", cfg->A);
    if (cfg->unit == SCTC_MBR_WORDS)
        SCTC_CHECK_ARG(cfg->space >= 1 && cfg->space < cfg->A, "nbest_mbr: space %d outside [1, %d)", cfg->space, cfg->A);
    SCTC_CHECK_ARG(std::isfinite(cfg->scale) && cfg->scale >= 0.0, "nbest_mbr: scale %g is not a finite number >= 0", cfg->scale);
    SCTC_CHECK_ARG(cfg->B == 0 || (cfg->K_b && cfg->U_b && cfg->label_off), "nbest_mbr: null K_b / U_b / label_off");
    for (int b = 0; b < cfg->B; ++b)
        SCTC_CHECK_ARG(cfg->K_b[b] >= 0 && cfg->K_b[b] <= cfg->K, "nbest_mbr: utterance %d has %d real hypotheses, outside 0..%d", b,
                       cfg->K_b[b], cfg->K);
    const int64_t P = (int64_t)cfg->B * cfg->K;
    SCTC_CHECK_ARG(P * cfg->K < (1ll << 31), "nbest_mbr: a distance matrix of %lld entries, the limit is 2^31 - 1", (long long)(P * cfg->K));
    int64_t slots = 0;
    for (int64_t o = 0; o < P; ++o) {
        SCTC_CHECK_ARG(cfg->U_b[o] >= 0 && cfg->U_b[o] <= MBR_MAX_U, "nbest_mbr: pair %lld has %d labels, outside 0..%d", (long long)o,
                       cfg->U_b[o], MBR_MAX_U);
        SCTC_CHECK_ARG(cfg->label_off[o] >= 0, "nbest_mbr: pair %lld has a negative offset", (long long)o);
        slots += intern_row_slots(cfg->U_b[o]);
    }
    SCTC_CHECK_ARG(slots < (1ll << 31), "nbest_mbr: %lld word slots, the limit is 2^31 - 1", (long long)slots);
    return SCTC_OK;
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_intern_words_workspace_bytes(const sctc_intern_config* cfg, size_t* bytes)
{
    SCTC_CHECK_ARG(bytes, "intern_words: null bytes");
    *bytes = 0;
    SCTC_TRY(check_intern(cfg));
    *bytes = intern_plan(cfg->N, cfg->U_b, cfg->label_off, cfg->G, cfg->group_off).bytes;
    return SCTC_OK;
}

int sctc_intern_words_batch(const sctc_intern_config* cfg, const int32_t* labels_dev, int32_t* word_ids_dev,
                            int32_t* counts_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream)
{
    SCTC_TRY(check_intern(cfg));
    if (cfg->N == 0) return SCTC_OK;
    const InternPlan pl = intern_plan(cfg->N, cfg->U_b, cfg->label_off, cfg->G, cfg->group_off);
    SCTC_CHECK_ARG(counts_dev && status_dev, "intern_words: null counts / status");
    SCTC_CHECK_ARG((labels_dev && word_ids_dev) || pl.n_slots == 0, "intern_words: null labels / word ids");
    if (workspace_bytes < pl.bytes || !workspace_dev)
        return set_error(SCTC_ERR_WORKSPACE, "intern_words: workspace %zu bytes < %zu needed",
                         workspace_dev ? workspace_bytes : (size_t)0, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    static thread_local PinnedStage* stage = new PinnedStage();
    char* pin = (char*)stage->acquire(pl.head_bytes);
    if (!pin) return set_error(SCTC_ERR_HIP, "intern_words: no pinned host memory for %zu bytes of descriptors", pl.head_bytes);
    intern_head(pl, pin);
    PinnedUploadGuard guard(s, true);
    SCTC_HIP_TRY(hipMemcpyAsync(ws, pin, pl.head_bytes, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();
    return launch_intern(pl, cfg->N, cfg->G, cfg->A, cfg->space, labels_dev, word_ids_dev, counts_dev, status_dev, ws, s);
}

int sctc_nbest_mbr_workspace_bytes(const sctc_mbr_config* cfg, size_t* bytes)
{
    SCTC_CHECK_ARG(bytes, "nbest_mbr: null bytes");
    *bytes = 0;
    SCTC_TRY(check_mbr(cfg));
    if (cfg->B == 0) return SCTC_OK;
    *bytes = mbr_plan(cfg->B, cfg->K, cfg->unit, cfg->flags, cfg->K_b, cfg->U_b, cfg->label_off).bytes;
    return SCTC_OK;
}

int sctc_nbest_mbr_batch(const sctc_mbr_config* cfg, const int32_t* labels_dev, const double* scores_dev,
                         const int32_t* order_dev, double* post_dev, double* risk_dev, int32_t* best_dev,
                         int32_t* mbr_order_dev, int32_t* dist_dev, double* conf_dev, int32_t* conf_len_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream)
{
    SCTC_TRY(check_mbr(cfg));
    if (cfg->B == 0) return SCTC_OK;
    const bool words = cfg->unit == SCTC_MBR_WORDS, conf = (cfg->flags & SCTC_MBR_CONF) != 0;
    SCTC_CHECK_ARG(scores_dev && post_dev && risk_dev && best_dev && mbr_order_dev, "nbest_mbr: null scores / outputs");
    SCTC_CHECK_ARG(!(cfg->flags & SCTC_MBR_DIST) || dist_dev, "nbest_mbr: SCTC_MBR_DIST without a distance matrix");
    SCTC_CHECK_ARG(!conf || conf_len_dev, "nbest_mbr: SCTC_MBR_CONF without conf_len");
    const MbrPlan pl = mbr_plan(cfg->B, cfg->K, cfg->unit, cfg->flags, cfg->K_b, cfg->U_b, cfg->label_off);
    bool any = false;
    for (int32_t v : pl.bound) any |= v > 0;
    SCTC_CHECK_ARG(labels_dev || !any, "nbest_mbr: null labels");
    SCTC_CHECK_ARG(!conf || conf_dev || pl.conf_slots == 0, "nbest_mbr: SCTC_MBR_CONF without conf");
    if (workspace_bytes < pl.bytes || !workspace_dev)
        return set_error(SCTC_ERR_WORKSPACE, "nbest_mbr: workspace %zu bytes < %zu needed", workspace_dev ? workspace_bytes : (size_t)0,
                         pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    const int32_t B = cfg->B, K = cfg->K;
    const int64_t P = (int64_t)B * K;

    // the descriptors: one image in the calling thread's pinned buffer, one copy per head
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t image = pl.head_bytes + (words ? pl.intern.head_bytes : 0);
    char* pin = (char*)stage->acquire(image);
    if (!pin) return set_error(SCTC_ERR_HIP, "nbest_mbr: no pinned host memory for %zu bytes of descriptors", image);
    memcpy(pin + pl.off_rows, pl.row_off.data(), (size_t)P * sizeof(int64_t));
    memcpy(pin + pl.off_utts, pl.utts.data(), (size_t)B * sizeof(MbrUtt));
    memcpy(pin + pl.off_kb, cfg->K_b, (size_t)B * sizeof(int32_t));
    memcpy(pin + pl.off_lens, pl.bound.data(), (size_t)P * sizeof(int32_t));    // word unit: overwritten by the counts
    if (words) intern_head(pl.intern, pin + pl.head_bytes);
    PinnedUploadGuard guard(s, true);
    SCTC_HIP_TRY(hipMemcpyAsync(ws, pin, pl.head_bytes, hipMemcpyHostToDevice, s));
    if (words)
        SCTC_HIP_TRY(hipMemcpyAsync(ws + pl.off_intern, pin + pl.head_bytes, pl.intern.head_bytes, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();

    MbrArgs a{};
    a.row_off = (const int64_t*)(ws + pl.off_rows);
    a.kb = (const int32_t*)(ws + pl.off_kb);
    a.lens = (const int32_t*)(ws + pl.off_lens);
    a.units = labels_dev;
    a.scores = scores_dev;
    a.order = order_dev;
    a.dist = (cfg->flags & SCTC_MBR_DIST) ? dist_dev : (int32_t*)(ws + pl.off_dist);
    a.post = post_dev;
    a.risk = risk_dev;
    a.best = best_dev;
    a.mbr_order = mbr_order_dev;
    a.scale = cfg->scale;
    a.B = B;
    a.K = K;
    if (conf) {
        a.w = (double*)(ws + pl.off_w);
        a.z = (double*)(ws + pl.off_z);
        a.match = (int8_t*)(ws + pl.off_match);
        a.ops = (int8_t*)(ws + pl.off_ops);
        a.tab = ws + pl.off_tab;
        a.tab_stride = pl.tab_stride;
        a.conf = conf_dev;
        a.conf_len = conf_len_dev;
    }
    if (words) {
        // the K ranks of an utterance are a group; a rank beyond K_b has no labels for the interning
        int32_t* ids = (int32_t*)(ws + pl.off_ids);
        SCTC_TRY(launch_intern(pl.intern, (int32_t)P, B, cfg->A, cfg->space, labels_dev, ids, (int32_t*)(ws + pl.off_lens),
                               (int32_t*)(ws + pl.off_status), ws + pl.off_intern, s));
        a.units = ids;
    }
    const int64_t cells = P * K;
    hipLaunchKernelGGL(nbest_fill_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    const int32_t n_alone = B - pl.n_common;
    const MbrUtt* utts = (const MbrUtt*)(ws + pl.off_utts);
    if (pl.pairs_common) {
        MbrArgs c = a;
        c.utts = utts;
        c.n_utts = pl.n_common;
        c.n_pairs = pl.pairs_common;
        c.slot = (int32_t)pl.slot_common;
        hipLaunchKernelGGL(nbest_dist_kernel, dim3((unsigned)((pl.pairs_common + WAVES - 1) / WAVES)), dim3(64 * WAVES),
                           WAVES * pl.slot_common, s, c);
        SCTC_HIP_TRY(hipGetLastError());
    }
    if (pl.pairs_alone) {       // a panel edge beyond 16 KB: one wave per workgroup
        MbrArgs c = a;
        c.utts = utts + pl.n_common;
        c.n_utts = n_alone;
        c.n_pairs = pl.pairs_alone;
        c.slot = (int32_t)pl.slot_alone;
        hipLaunchKernelGGL(nbest_dist_kernel, dim3((unsigned)pl.pairs_alone), dim3(64), pl.slot_alone, s, c);
        SCTC_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(nbest_mbr_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, a);
    SCTC_HIP_TRY(hipGetLastError());
    if (!conf) return SCTC_OK;
    if (pl.n_common) {
        MbrArgs c = a;
        c.utts = utts;
        c.n_utts = pl.n_common;
        c.slot = (int32_t)pl.cslot_common;
        const int64_t waves = (int64_t)pl.n_common * K;
        hipLaunchKernelGGL(nbest_conf_kernel, dim3((unsigned)((waves + WAVES - 1) / WAVES)), dim3(64 * WAVES),
                           WAVES * pl.cslot_common, s, c);
        SCTC_HIP_TRY(hipGetLastError());
    }
    if (n_alone) {
        MbrArgs c = a;
        c.utts = utts + pl.n_common;
        c.n_utts = n_alone;
        c.slot = (int32_t)pl.cslot_alone;
        hipLaunchKernelGGL(nbest_conf_kernel, dim3((unsigned)((int64_t)n_alone * K)), dim3(64), pl.cslot_alone, s, c);
        SCTC_HIP_TRY(hipGetLastError());
    }
    MbrArgs c = a;
    c.utts = utts;
    c.n_utts = B;
    hipLaunchKernelGGL(nbest_conf_sum_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, c);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
