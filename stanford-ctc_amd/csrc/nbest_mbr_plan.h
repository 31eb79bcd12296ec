// How sctc_intern_words_batch and sctc_nbest_mbr_batch (nbest_mbr.hip) lay out their workspaces and
// choose their launches: pure functions of plain integers (host only, no HIP header: tests/test_mbr_plan_cpu.py compiles
// this file with g++).  nbest_mbr.hip validates, plans, uploads and launches; its kernels decide nothing.
//
// Interning.  Row n owns the word slots from sum_{q<n} ceil(U_b[q] / 2): a row of U symbols has at most ceil(U / 2)
// words.  A group owns a hash table of 32-bit slot indices, a power of two of at least twice its slots (no table for a
// group without slots).  Workspace, every slice rounded up to 256 bytes, in this order:
//   rows     N descriptors of 32 bytes                         | uploaded
//   groups   G descriptors of 8 bytes (first row, end row)     | uploaded
//   base     N int32: the tokens of the group's earlier rows
//   meta     24 bytes per slot: where the token lies, its length and hash, its row
//   table    4 bytes per table entry                           | meta and table are one span, filled with 0xff
//
// MBR.  Pair (b, k) at b * K + k.  The bound of a row is what the host knows of its unit count: U_b in character
// unit, ceil(U_b / 2) in word unit, 0 for a rank k >= K_b[b].  An utterance has K_b (K_b - 1) / 2 pairs; its waves need
// an LDS slot of 32 bytes (the five counts of edit_pair, the path's length) plus, when its longest bound is beyond one panel of 256
// columns, 8 bytes per row of a for the panel edge.  Utterances whose slot fits 16 KB run four waves to a workgroup
// (the common launch), the others one wave to a workgroup (alone), as plan_edit of edit_distance.hip does pair by pair.
// Workspace, every slice rounded up to 256 bytes, in this order:
//   rows     B * K int64: first unit of the row (label_off, or the row's first word slot)        | uploaded
//   utts     B descriptors of 32 bytes, the common launch's first, each with its first pair      | uploaded
//   kb       B int32: K_b                                                                         | uploaded
//   lens     B * K int32: the unit counts (character unit: uploaded; word unit: the interning's counts)
//   status   B * K int32, word unit only: the interning's status
//   ids      one int32 per word slot, word unit only
//   intern   the interning's own workspace, word unit only
//   dist     B * K * K int32, unless the caller keeps the distances (SCTC_MBR_DIST)
//   conf     with SCTC_MBR_CONF: B * K double weights | B double normalisers | match flags, one byte per unit of the
//            longest bound of b for every pair (b, j) | the paths, twice as many bytes | one operation table per pair
//            of the size that the largest table needs that does not fit its wave's LDS slot (none: nothing)
// Confidences.  Utterance b owns the slots from sum_{q<b} longest bound of q.  A confidence wave aligns the chosen
// hypothesis (a) with hypothesis j (b): its LDS slot holds the counts, the panel edge and, when it fits, the 2-bit
// operation table; the launches and their order of utterances are those of the distances.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sctc {

constexpr int MBR_CHARS = 0, MBR_WORDS = 1;     // SCTC_MBR_* of include/sctc.h
constexpr int MBR_FLAG_CONF = 1, MBR_FLAG_DIST = 2;
constexpr int MBR_MAX_K = 256;
constexpr int MBR_MAX_U = 4095;                 // ALIGN_MAX_U: these rows have been aligned
constexpr int MBR_PANEL = 256;                  // PANEL of edit_dev.h
constexpr size_t MBR_SLOT_MAX = 16384;          // SLOT_MAX of edit_dev.h
constexpr size_t MBR_STAT_BYTES = 32;           // the five counts of edit_pair and the path's length, in front of the panel edge
constexpr int MBR_WAVES = 4;

static inline size_t mbr_align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct InternRow {
    int64_t label_off;  // first label in labels_dev
    int64_t slot_off;   // first word slot
    int64_t tab_off;    // first entry of the group's table
    int32_t U;
    uint32_t tab_mask;  // entries - 1; not read for a row without slots
};

struct InternGroup {
    int32_t first, end; // rows [first, end)
};

struct InternMeta {     // one per word slot; len < 0 (the 0xff fill): no token here
    int64_t off;        // first symbol in labels_dev
    int32_t len;
    uint32_t hash;
    int32_t row;
    int32_t pad;        // keeps the struct at 24 bytes; the word's table entry waits in its id slot, not here
};

struct InternPlan {
    std::vector<InternRow> rows;
    std::vector<InternGroup> groups;
    int64_t n_slots = 0, n_table = 0;
    size_t off_rows = 0, off_groups = 0, head_bytes = 0, off_base = 0, off_meta = 0, off_table = 0, fill_bytes = 0;
    size_t bytes = 0;
};

static inline int64_t intern_row_slots(int32_t U) { return (U + 1) / 2; }

// U_b / label_off: N rows; group_off [G + 1]: non-decreasing, group_off[0] = 0, group_off[G] = N (validated by the caller)
static inline InternPlan intern_plan(int32_t N, const int32_t* U_b, const int64_t* label_off, int32_t G,
                                     const int32_t* group_off)
{
    InternPlan p;
    p.rows.resize(N);
    p.groups.resize(G);
    int64_t slot = 0, tab = 0;
    for (int32_t g = 0; g < G; ++g) {
        p.groups[g] = InternGroup{group_off[g], group_off[g + 1]};
        int64_t s = 0;
        for (int32_t n = group_off[g]; n < group_off[g + 1]; ++n) s += intern_row_slots(U_b[n]);
        int64_t cap = 0;
        if (s > 0) {
            cap = 2;
            while (cap < 2 * s) cap *= 2;
        }
        for (int32_t n = group_off[g]; n < group_off[g + 1]; ++n) {
            p.rows[n] = InternRow{label_off[n], slot, tab, U_b[n], (uint32_t)(cap ? cap - 1 : 0)};
            slot += intern_row_slots(U_b[n]);
        }
        tab += cap;
    }
    p.n_slots = slot;
    p.n_table = tab;
    size_t at = 0;
    p.off_rows = at;
    at += mbr_align256((size_t)N * sizeof(InternRow));
    p.off_groups = at;
    at += mbr_align256((size_t)G * sizeof(InternGroup));
    p.head_bytes = at;
    p.off_base = at;
    at += mbr_align256((size_t)N * sizeof(int32_t));
    p.off_meta = at;
    at += mbr_align256((size_t)slot * sizeof(InternMeta));
    p.off_table = at;
    at += mbr_align256((size_t)tab * sizeof(uint32_t));
    p.fill_bytes = at - p.off_meta;
    p.bytes = at;
    return p;
}

struct MbrUtt {
    int64_t pair_off;   // first pair of the utterance in its launch
    int64_t conf_off;   // first confidence slot: the longest bounds of the utterances before it
    int32_t b;
    int32_t kb;
    int32_t longest;    // longest bound of its real ranks
    int32_t pad;
};

struct MbrPlan {
    std::vector<int64_t> row_off;   // [B * K]
    std::vector<int32_t> bound;     // [B * K]
    std::vector<MbrUtt> utts;       // [B]: the common launch's, then the others
    int32_t n_common = 0;           // utterances of the common launch
    int64_t pairs_common = 0, pairs_alone = 0;
    size_t slot_common = 0, slot_alone = 0;
    InternPlan intern;              // word unit
    // confidences
    int64_t conf_slots = 0;         // sum of the longest bounds
    size_t cslot_common = 0, cslot_alone = 0;   // LDS of a confidence wave: counts, panel edge, operation table if it fits
    size_t tab_stride = 0;          // bytes of one pair's operation table in the workspace (0: all fit in LDS)
    size_t off_rows = 0, off_utts = 0, off_kb = 0, off_lens = 0, head_bytes = 0, off_status = 0, off_ids = 0, off_intern = 0,
           off_dist = 0, off_w = 0, off_z = 0, off_match = 0, off_ops = 0, off_tab = 0;
    size_t bytes = 0;
};

// LDS of one wave for a pair whose a has up to n and whose b up to m units: the counts, and the panel edge
static inline size_t mbr_pair_slot(int32_t n, int32_t m)
{
    return MBR_STAT_BYTES + (n > 0 && m > MBR_PANEL ? (size_t)n * 8 : 0);
}

// bytes of the 2-bit operation table of such a pair (edit_pair<true>)
static inline size_t mbr_pair_table(int32_t n, int32_t m)
{
    return n > 0 && m > 0 ? (size_t)((n + 3) / 4) * ((m + 3) / 4) * 4 : 0;
}

// K_b [B], U_b / label_off [B * K] validated by the caller
static inline MbrPlan mbr_plan(int32_t B, int32_t K, int32_t unit, int32_t flags, const int32_t* K_b, const int32_t* U_b,
                               const int64_t* label_off)
{
    MbrPlan p;
    const int64_t P = (int64_t)B * K;
    p.row_off.resize(P);
    p.bound.resize(P);
    std::vector<int32_t> eff(P);        // lengths that the interning sees: nothing of a rank beyond K_b is read
    for (int64_t o = 0; o < P; ++o) {
        const bool in = (int32_t)(o % K) < K_b[o / K];
        eff[o] = in ? U_b[o] : 0;
        p.bound[o] = unit == MBR_WORDS ? (int32_t)intern_row_slots(eff[o]) : eff[o];
    }
    if (unit == MBR_WORDS) {
        std::vector<int32_t> goff(B + 1);
        for (int32_t b = 0; b <= B; ++b) goff[b] = b * K;
        p.intern = intern_plan((int32_t)P, eff.data(), label_off, B, goff.data());
        for (int64_t o = 0; o < P; ++o) p.row_off[o] = p.intern.rows[o].slot_off;
    } else {
        for (int64_t o = 0; o < P; ++o) p.row_off[o] = label_off[o];
    }
    const bool conf = (flags & MBR_FLAG_CONF) != 0;
    std::vector<MbrUtt> alone;
    std::vector<int32_t> longest(B);
    size_t tab_max = 0;
    for (int32_t b = 0; b < B; ++b) {
        int32_t mx = 0;
        for (int32_t k = 0; k < K_b[b]; ++k) mx = std::max(mx, p.bound[(int64_t)b * K + k]);
        longest[b] = mx;
        const size_t need = mbr_pair_slot(mx, mx);
        MbrUtt u{0, p.conf_slots, b, K_b[b], mx, 0};
        p.conf_slots += mx;
        if (need <= MBR_SLOT_MAX) {
            p.slot_common = std::max(p.slot_common, need);
            p.utts.push_back(u);
        } else {
            p.slot_alone = std::max(p.slot_alone, need);
            alone.push_back(u);
        }
        if (conf) {
            // a confidence wave keeps the operation table behind the edge when both fit the slot of its launch;
            // whether they do is decided per launch from the longest bound in it, so that one stride serves all
            const size_t tab = mbr_pair_table(mx, mx);
            size_t& cs = need <= MBR_SLOT_MAX ? p.cslot_common : p.cslot_alone;
            if (need + tab <= MBR_SLOT_MAX) cs = std::max(cs, need + tab);
            else {
                cs = std::max(cs, need);
                tab_max = std::max(tab_max, tab);
            }
        }
    }
    p.n_common = (int32_t)p.utts.size();
    p.utts.insert(p.utts.end(), alone.begin(), alone.end());
    for (int32_t i = 0; i < B; ++i) {
        MbrUtt& u = p.utts[i];
        int64_t& run = i < p.n_common ? p.pairs_common : p.pairs_alone;
        u.pair_off = run;
        run += (int64_t)u.kb * (u.kb - 1) / 2;
    }
    p.slot_common = (p.slot_common + 15) & ~(size_t)15;
    p.slot_alone = (p.slot_alone + 15) & ~(size_t)15;
    p.cslot_common = (p.cslot_common + 15) & ~(size_t)15;
    p.cslot_alone = (p.cslot_alone + 15) & ~(size_t)15;
    p.tab_stride = mbr_align256(tab_max);

    size_t at = 0;
    p.off_rows = at;
    at += mbr_align256((size_t)P * sizeof(int64_t));
    p.off_utts = at;
    at += mbr_align256((size_t)B * sizeof(MbrUtt));
    p.off_kb = at;
    at += mbr_align256((size_t)B * sizeof(int32_t));
    p.off_lens = at;
    at += mbr_align256((size_t)P * sizeof(int32_t));
    p.head_bytes = at;
    p.off_status = at;
    if (unit == MBR_WORDS) at += mbr_align256((size_t)P * sizeof(int32_t));
    p.off_ids = at;
    if (unit == MBR_WORDS) at += mbr_align256((size_t)p.intern.n_slots * sizeof(int32_t));
    p.off_intern = at;
    if (unit == MBR_WORDS) at += p.intern.bytes;
    p.off_dist = at;
    if (!(flags & MBR_FLAG_DIST)) at += mbr_align256((size_t)P * K * sizeof(int32_t));
    p.off_w = at;
    if (conf) {
        at += mbr_align256((size_t)P * sizeof(double));
        p.off_z = at;
        at += mbr_align256((size_t)B * sizeof(double));
        p.off_match = at;
        int64_t units = 0;
        for (int32_t b = 0; b < B; ++b) units += (int64_t)K * longest[b];
        at += mbr_align256((size_t)units);
        p.off_ops = at;
        at += mbr_align256((size_t)units * 2);
        p.off_tab = at;
        at += (size_t)P * p.tab_stride;
    }
    p.bytes = at;
    return p;
}

}  // namespace sctc
