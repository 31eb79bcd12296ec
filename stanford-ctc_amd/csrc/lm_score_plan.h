// How sctc_lm_score_batch (lm_score.hip) walks a batch of label sequences and how its workspace is
// laid out: pure functions of plain integers (host only, no HIP header: tests/test_lm_score_plan_cpu.py compiles this
// file with g++).  lm_score.hip validates, plans, uploads and launches; its kernels decide nothing.
//
//   recurrent LM      a tile is up to 32 WHOLE sequences that one workgroup walks in lockstep.  The sequences are
//                     ordered by descending length, stably, and cut into tiles in that order: the slots of a tile that
//                     are still alive at step t are then always the prefix 0..cnt_t-1, which is what rnnlm_tile's
//                     `cnt` wants.  A tile runs as many steps as its longest (= first) sequence has labels.
//   window / n-gram   positions are independent: the descriptors stay in the caller's order, a tile is 32 consecutive
//                     positions of the flattened list (window LM), a lane owns one position (n-gram LM).
//
// Workspace, every slice rounded up to 256 bytes, in this order:
//   seqs     N descriptors of 24 bytes
//   tiles    the recurrent LM's tiles, 16 bytes each
//   symbols  A int32: the LM id of every symbol
//   terms    sum U float32, only when the caller passes no terms array
//   scratch  `resident` tiles of tile_bytes each (recurrent: rnn_tile_bytes + two [32][H] state buffers; window:
//            nn_tile_bytes; n-gram: nothing), resident = min(tiles, LM_SCORE_RESIDENT)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sctc {

constexpr int LM_SCORE_NGRAM = 0, LM_SCORE_NN = 1, LM_SCORE_RNN = 2;   // SCTC_LM_* of include/sctc.h
constexpr int LM_SCORE_TILE = 32;           // NN_TILE of nnlm_dev.h
constexpr int LM_SCORE_RESIDENT = 512;      // workgroups, and tiles of scratch, of the two neural paths
constexpr int LM_SCORE_MAX_U = 8191;
constexpr int LM_SCORE_NGRAM_THREADS = 256; // one position per lane

struct LmSeq {
    int64_t label_off;   // first label in labels_dev
    int64_t term_off;    // first term: sum of the lengths of the caller's earlier sequences
    int32_t U;
    int32_t n;           // index in the caller's order
};

struct LmTile {
    int32_t first;       // first descriptor of the tile
    int32_t cnt;         // 1..32 sequences
    int32_t steps;       // labels of its longest sequence
    int32_t pad;
};

struct LmScorePlan {
    std::vector<LmSeq> seqs;
    std::vector<LmTile> tiles;      // recurrent LM only
    int64_t n_terms = 0;
    int64_t n_tiles = 0;            // of the neural paths (window LM: tiles of positions)
    int32_t resident = 0;
    int32_t grid = 0;               // workgroups of the path's kernel
    size_t off_seqs = 0, off_tiles = 0, off_sym = 0, off_terms = 0, off_scratch = 0;
    size_t bytes = 0;
};

static inline size_t lm_score_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// kind: LM_SCORE_*; U_b / label_off: the caller's N sequences (already validated); tile_bytes: scratch of one resident
// tile; terms_in_ws: the caller passed no terms array
static inline LmScorePlan lm_score_plan(int kind, int32_t N, int32_t A, const int32_t* U_b, const int64_t* label_off,
                                        size_t tile_bytes, bool terms_in_ws)
{
    LmScorePlan p;
    p.seqs.resize(N);
    int64_t off = 0;
    for (int32_t n = 0; n < N; ++n) {
        p.seqs[n] = LmSeq{label_off ? label_off[n] : 0, off, U_b[n], n};
        off += U_b[n];
    }
    p.n_terms = off;
    if (kind == LM_SCORE_RNN) {
        std::stable_sort(p.seqs.begin(), p.seqs.end(), [](const LmSeq& a, const LmSeq& b) { return a.U > b.U; });
        // sequences without labels have no step to take: they sort last and get no tile
        int32_t live = 0;
        while (live < N && p.seqs[live].U > 0) ++live;
        for (int32_t f = 0; f < live; f += LM_SCORE_TILE)
            p.tiles.push_back(LmTile{f, std::min<int32_t>(LM_SCORE_TILE, live - f), p.seqs[f].U, 0});
        p.n_tiles = (int64_t)p.tiles.size();
    } else if (kind == LM_SCORE_NN) {
        p.n_tiles = (p.n_terms + LM_SCORE_TILE - 1) / LM_SCORE_TILE;
    }
    if (kind == LM_SCORE_NGRAM) {
        p.resident = 0;
        p.grid = (int32_t)std::min<int64_t>((p.n_terms + LM_SCORE_NGRAM_THREADS - 1) / LM_SCORE_NGRAM_THREADS, 1 << 20);
    } else {
        p.resident = (int32_t)std::min<int64_t>(p.n_tiles, LM_SCORE_RESIDENT);
        p.grid = p.resident;
    }
    size_t at = 0;
    p.off_seqs = at;
    at += lm_score_align256((size_t)N * sizeof(LmSeq));
    p.off_tiles = at;
    at += lm_score_align256(p.tiles.size() * sizeof(LmTile));
    p.off_sym = at;
    at += lm_score_align256((size_t)A * sizeof(int32_t));
    p.off_terms = at;
    if (terms_in_ws) at += lm_score_align256((size_t)p.n_terms * sizeof(float));
    p.off_scratch = at;
    at += (size_t)p.resident * tile_bytes;
    p.bytes = at;
    return p;
}

}  // namespace sctc
