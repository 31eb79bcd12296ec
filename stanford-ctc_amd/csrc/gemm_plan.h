// Which GEMM kernel a call runs, on which tile, with how many K slices and how much split-K workspace: pure functions
// of plain integers (host only, no HIP header: tests/test_gemm_plan_cpu.py compiles this file with g++ and compares
// every decision with a recorded table).  launch_gemm_f32 (gemm_f32.hip) validates, plans and launches; gemm_f32.hip,
// gemm_h16.hip, gemm_g16.hip and gemm_s3.hip turn a plan into a template instantiation and decide nothing; the kernels'
// own tile constants are tied to the tables below by static_asserts next to them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

namespace sctc {

// ---------------------------------------------------------------- the switches ("switches")

struct GemmSwitches {
    int shape = -1;      // SCTC_GEMM_SHAPE=0..3: forces the fp32 kernel's tile shape (-1: least padded work)
    int h16_tile = -1;   // SCTC_H16_TILE=0 / 1: forces the 128 / 256 tile of the 16-bit kernels (-1: by output size)
    int g16 = 1;         // SCTC_G16=0: the register-staged 16-bit kernel instead of the LDS-DMA one
};

// The one reader of the environment in the GEMM sources; once per plan (tests flip switches between calls).
static inline GemmSwitches gemm_switches_from_env()
{
    GemmSwitches s;
    const char* v;
    if ((v = getenv("SCTC_GEMM_SHAPE"))) s.shape = atoi(v) < 0 ? 0 : (atoi(v) > 3 ? 3 : atoi(v));
    if ((v = getenv("SCTC_H16_TILE"))) s.h16_tile = atoi(v) ? 1 : 0;
    if ((v = getenv("SCTC_G16"))) s.g16 = atoi(v) != 0;
    return s;
}

// ---------------------------------------------------------------- what a decision may depend on

// The plain facts of a GemmArgs (gemm_f32.h, gemm_query): no pointers, so that every decision can be replayed on a CPU.
struct GemmQuery {
    int M = 0, N = 0, K = 0;
    int prec = 0, in16 = 0;              // GemmArgs::prec / in16
    int a_kcontig = 0, b_kcontig = 0;
    bool idx_a = false, idx_b = false;   // a row gather is set
    bool a2 = false;                     // the two-addend A operand
    int lda_mod8 = 0, ldb_mod8 = 0;
    // gemm_validate only
    bool a_sum = false, shadows = false, skip_c32 = false, accumulate = false, mask = false, mask16 = false;
    bool ab_misaligned = false, a2_misaligned = false;   // A or B / A2 or a_sum off a 16-byte boundary
    int ldmask16_mod4 = 0;
    int splits = 1;
    bool workspace = false;
};

// The argument checks of launch_gemm_f32, in its order: false and the message in `why`.
static inline bool gemm_validate(const GemmQuery& q, char* why, size_t n)
{
    const auto fail = [&](const char* msg) { snprintf(why, n, "%s", msg); return false; };
    if (q.K < 0) return fail("gemm: negative K");
    if (q.lda_mod8 % 4 != 0 || q.ldb_mod8 % 4 != 0) return fail("gemm: lda/ldb must be multiples of 4");
    if (q.ab_misaligned) return fail("gemm: operands must be 16-byte aligned");
    if (q.in16) {
        if (!(q.prec != 0 && q.a_kcontig == q.b_kcontig && q.lda_mod8 == 0 && q.ldb_mod8 == 0 && (!q.a_kcontig || q.K % 8 == 0)))
            return fail("gemm: 16-bit operands need prec != 0, equal operand layouts, lda/ldb % 8 == 0 "
                        "and (K-contiguous) K % 8 == 0");
    } else if (q.shadows && q.prec == 0) {
        return fail("gemm: 16-bit shadow outputs need prec != 0");
    }
    if (q.skip_c32 && !(q.shadows && !q.accumulate && q.prec != 0))
        return fail("gemm: skip_c32 needs a 16-bit shadow output, no accumulate and prec != 0");
    if (q.mask16 && !(!q.mask && q.prec != 0 && q.ldmask16_mod4 == 0)) return fail("gemm: mask16 excludes mask, needs prec != 0");
    if (q.a_kcontig && q.K % 4 != 0) return fail("gemm: K must be a multiple of 4 (A K-contig)");
    if (!q.a_kcontig && q.M % 4 != 0) return fail("gemm: M must be a multiple of 4 (A row-contig)");
    if (q.b_kcontig && q.K % 4 != 0) return fail("gemm: K must be a multiple of 4 (B K-contig)");
    if (!q.b_kcontig && q.N % 4 != 0) return fail("gemm: N must be a multiple of 4 (B row-contig)");
    if (q.a2 && !(q.prec == 0 && q.a_kcontig == q.b_kcontig && !q.idx_a && !q.a2_misaligned))
        return fail("gemm: a two-addend A operand needs prec 0, layout NT or TN, no row gather, 16-byte alignment");
    if (q.a_sum && !q.a2) return fail("gemm: a_sum without A2");
    if (q.splits > 1 && !q.workspace) return fail("gemm: split-K without workspace");
    if (q.prec < 0 || q.prec > 3) {
        snprintf(why, n, "gemm: unknown operand precision %d", q.prec);
        return false;
    }
    if (q.prec == 3 && (q.in16 || q.shadows)) return fail("gemm: the three-term split takes fp32 operands and writes no 16-bit shadows");
    return true;
}

// ---------------------------------------------------------------- the tile tables

#ifndef SCTC_GEMM_BK
#define SCTC_GEMM_BK 16
#endif
#ifndef SCTC_GEMM_OCC
#define SCTC_GEMM_OCC 3
#endif
#ifndef SCTC_GEMM_OCC1
#define SCTC_GEMM_OCC1 4
#endif

// the fp32 kernel's block tiles (gemm_f32.hip, TileCfg<i>); `penalty`: what a smaller tile must save in padded work
struct GemmShape { int bm, bn, occ; double penalty; };
static constexpr int GEMM_N_SHAPES = 4;
constexpr GemmShape gemm_shape(int i)
{
    return i == 0 ? GemmShape{128, 128, SCTC_GEMM_OCC, 0.00}
         : i == 1 ? GemmShape{128, 96, SCTC_GEMM_OCC1, 0.02}
         : i == 2 ? GemmShape{64, 128, 4, 0.10}
                  : GemmShape{128, 64, 4, 0.10};
}
static constexpr int GEMM_F32_BK = SCTC_GEMM_BK;
// the 16-bit kernels (gemm_h16.hip, HTile<big>; gemm_g16.hip) and the three-term split (gemm_s3.hip)
constexpr int gemm_h16_tile(bool big) { return big ? 256 : 128; }
static constexpr int GEMM_H16_BK = 32, GEMM_X16_BK = 64, GEMM_G16_BK = 32, GEMM_G16_LDS = 139264;
static constexpr int GEMM_S3_TILE = 128, GEMM_S3_BK = 16, GEMM_S3_LDS = 73728;
// the split-K search of every kernel but the fp32 one counts K tiles of 64, whatever the kernel's own K tile
static constexpr int GEMM_SPLIT_BK16 = 64;

// fp32: the tile shape with the least padded (wasted) matrix-core work for an M x N output
static inline int gemm_pick_shape(int M, int N, const GemmSwitches& sw)
{
    if (sw.shape >= 0) return sw.shape;
    int best = 0;
    double best_cost = 1e30;
    for (int i = 0; i < GEMM_N_SHAPES; ++i) {
        const GemmShape s = gemm_shape(i);
        const double pm = (double)((M + s.bm - 1) / s.bm * s.bm) / M;
        const double pn = (double)((N + s.bn - 1) / s.bn * s.bn) / N;
        const double cost = pm * pn + s.penalty;
        if (cost < best_cost - 1e-12) { best_cost = cost; best = i; }
    }
    return best;
}

// 16-bit kernels: the 256x256 tile when the output is large enough to give every CU whole tiles of it and its padding
// does not cost more than it saves (H = 1824 = 7.1 x 256 pads 12 %)
static inline bool gemm_h16_pick_big(int M, int N, int K, bool g16, const GemmSwitches& sw)
{
    if (sw.h16_tile >= 0) return sw.h16_tile != 0;
    const auto padded = [](int v, int t) { return (double)((v + t - 1) / t * t) / v; };
    const double small = padded(M, 128) * padded(N, 128), big = padded(M, 256) * padded(N, 256);
    const int64_t tiles_big = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
    // the LDS-DMA kernel runs the long-K weight gradients at twice the rate of the 128 x 128 register-staged one
    // (cfg-5 input layer, 2048 x 640 x 64000: 0.63 ms there): it may waste up to 25 % on padding and fills the
    // machine through split-K
    if (g16 && K >= 4096 && tiles_big >= 8 && big <= 1.25 * small) return true;
    return tiles_big >= 32 && big <= 1.06 * small;
}

// ---------------------------------------------------------------- split-K

// 256 CUs x `occ` resident blocks.  A grid that is not a multiple of that leaves a partial last round (225 tiles x
// 3 splits = 675 blocks ran at 66 %): the split that fills whole rounds best, keeping >= min_ktiles K tiles per split.
static inline int gemm_split_search(int tiles, int slots, int ktiles, int min_ktiles)
{
    int s = 1;
    if (tiles < 2 * slots) {
        double best = 0.0;
        const int by_k = ktiles / min_ktiles, smax = by_k < 1 ? 1 : (by_k > 64 ? 64 : by_k);
        for (int c = 1; c <= smax; ++c) {
            const int blocks = tiles * c;
            const int rounds = (blocks + slots - 1) / slots;
            // efficiency of the last round, mildly penalising the extra partial traffic
            const double eff = (double)blocks / ((double)rounds * slots) - 0.002 * c;
            if (eff > best + 1e-9) { best = eff; s = c; }
        }
    }
    return s;
}

// partials [splits][M][N], then [splits][M] column-sum partials
static inline int64_t gemm_split_floats(int splits, int M, int N) { return splits > 1 ? (int64_t)splits * M * (N + 1) : 0; }

// ---------------------------------------------------------------- the plan

enum GemmKernel {
    GEMM_F32,   // gemm_f32.hip: fp32 MFMA
    GEMM_H16,   // gemm_h16.hip, gemm_h16_kernel: fp32 operands rounded to 16 bit in registers
    GEMM_X16,   // gemm_h16.hip, gemm_x16_kernel: 16-bit operands in memory, staged through registers
    GEMM_G16,   // gemm_g16.hip: 16-bit operands in memory, staged by LDS-DMA
    GEMM_S3,    // gemm_s3.hip: fp32 operands as three bfloat16 terms
};

struct GemmPlan {
    GemmKernel kernel = GEMM_F32;
    int bm = 0, bn = 0, bk = 0, threads = 0, lds_bytes = 0;
    int grid_x = 0;          // output tiles; grid.y is GemmArgs::splits
    // What the caller should put into GemmArgs::splits when it has ws_floats of workspace (else 1).
    int splits = 1;
    int64_t ws_floats = 0;
    int occ = 0;             // resident blocks per CU the split search counted on
    // KNOWN ODDITY, kept as found: the split search of the 16-bit kernels picks ITS tile from the hint "16-bit
    // operands of one layout, A not gathered", the kernel picks its own from the exact LDS-DMA predicate, which also
    // wants B ungathered and, row-contiguous, M % 8 == N % 8 == 0.  Where the two disagree (true here) `splits`
    // was computed for a 256 tile of one block per CU and runs on 128 tiles, or the reverse; ws_floats holds either way.
    bool split_tile_differs = false;
    // template selectors of the launchers
    int shape = 0;           // GEMM_F32: gemm_shape index
    bool big = false;        // GEMM_H16 / GEMM_X16: the 256 tile
    bool bf = false;         // 16-bit kernels: bfloat16 (prec 2), else float16
    bool ak = false, bkc = false;   // operand layouts (K-contiguous)
    bool gather = false;     // GEMM_S3: a row-contiguous operand is gathered
    bool a2 = false;         // GEMM_F32: two-addend A operand
};

static inline GemmPlan gemm_plan(const GemmQuery& q, const GemmSwitches& sw)
{
    GemmPlan p;
    p.ak = q.a_kcontig != 0;
    p.bkc = q.b_kcontig != 0;
    p.bf = q.prec == 2;
    p.a2 = q.a2;
    p.gather = (q.idx_a && !q.a_kcontig) || (q.idx_b && !q.b_kcontig);
    int split_tile_m, split_tile_n, split_bk = GEMM_SPLIT_BK16, min_ktiles = 4;
    if (q.prec == 0) {
        p.kernel = GEMM_F32;
        p.shape = gemm_pick_shape(q.M, q.N, sw);
        const GemmShape s = gemm_shape(p.shape);
        p.bm = split_tile_m = s.bm;
        p.bn = split_tile_n = s.bn;
        p.bk = split_bk = GEMM_F32_BK;
        min_ktiles = 8;
        p.occ = s.occ;
        p.threads = 256;
        p.lds_bytes = 4 * 2 * GEMM_F32_BK * (s.bm + 4 + s.bn + 4);   // 2 buffers, rows padded by 4
    } else if (q.prec == 3) {
        p.kernel = GEMM_S3;
        p.bm = p.bn = split_tile_m = split_tile_n = GEMM_S3_TILE;
        p.bk = GEMM_S3_BK;
        p.occ = 2;
        p.threads = 256;
        p.lds_bytes = GEMM_S3_LDS;
    } else {
        const bool hint = q.in16 && q.a_kcontig == q.b_kcontig && !q.idx_a && sw.g16;
        const bool g16 = hint && !q.idx_b && q.lda_mod8 == 0 && q.ldb_mod8 == 0 &&
                         (q.a_kcontig ? q.K % 8 == 0 : (q.M % 8 == 0 && q.N % 8 == 0));
        const bool split_big = gemm_h16_pick_big(q.M, q.N, q.K, hint, sw);
        p.big = gemm_h16_pick_big(q.M, q.N, q.K, g16, sw);
        p.split_tile_differs = split_big != p.big;
        p.kernel = (p.big && g16) ? GEMM_G16 : (q.in16 ? GEMM_X16 : GEMM_H16);
        p.bm = p.bn = gemm_h16_tile(p.big);
        split_tile_m = split_tile_n = gemm_h16_tile(split_big);
        p.occ = split_big ? 1 : 2;
        p.threads = p.big ? 512 : 256;
        p.bk = p.kernel == GEMM_G16 ? GEMM_G16_BK : (p.kernel == GEMM_X16 ? GEMM_X16_BK : GEMM_H16_BK);
        p.lds_bytes = p.kernel == GEMM_G16 ? GEMM_G16_LDS : 2 * 2 * (p.bm + p.bn) * (p.bk + 8);   // rows of bk + 8 halves
    }
    p.grid_x = ((q.M + p.bm - 1) / p.bm) * ((q.N + p.bn - 1) / p.bn);
    const int tiles = ((q.M + split_tile_m - 1) / split_tile_m) * ((q.N + split_tile_n - 1) / split_tile_n);
    p.splits = gemm_split_search(tiles, 256 * p.occ, (q.K + split_bk - 1) / split_bk, min_ktiles);
    p.ws_floats = gemm_split_floats(p.splits, q.M, q.N);
    return p;
}

// ---------------------------------------------------------------- the engine's split-K workspace (brnn_engine.hip, carve)

// Floats of split-K partials a network of these padded layer widths gets at create time, for up to F frames per
// minibatch: the worst case over the weight-gradient GEMMs (K = frames) at K = F; and, because small minibatches (few row
// tiles) split K in the forward / delta-propagation GEMMs as well, 64 slices of those -- but at most BRNN_SPLITK_CAP:
// blocks x splits stays below ~2 rounds of resident blocks, i.e. <= 2 * 1024 tiles of 128 x 128.
// The engine takes a planned split only where the plan's ws_floats fits (brnn_engine.hip, launch_gemm).
// tests/test_gemm_plan_cpu.py: this covers every weight-gradient plan, for every K up to F, contiguous or gathered; the
// forward / delta plans it does not cover are exactly those above the cap, which therefore run unsplit.
static constexpr int64_t BRNN_SPLITK_CAP = (int64_t)2 * 1024 * 128 * 128;
static inline int64_t brnn_splitk_floats(int Dp, int Hp, int Ap, int NL, bool temporal, int64_t F, bool train, int bwd_prec,
                                         int in16, const GemmSwitches& sw)
{
    int64_t sk = 0;
    const auto wgrad = [&](int outp, int inp) {
        const int64_t need = gemm_plan(GemmQuery{outp, inp, (int)F, bwd_prec, in16, 0, 0}, sw).ws_floats;
        if (need > sk) sk = need;
    };
    if (train) {
        for (int l = 0; l <= NL; ++l) wgrad(l == NL ? Ap : Hp, l == 0 ? Dp : Hp);
        if (temporal) wgrad(Hp, Hp);
    }
    const int64_t small = (int64_t)64 * F * ((Hp > Ap ? Hp : Ap) + 1), floor_ = small < BRNN_SPLITK_CAP ? small : BRNN_SPLITK_CAP;
    return sk > floor_ ? sk : floor_;
}

}  // namespace sctc
