// Which CTC kernel a batch runs and how its workspace is laid out: pure functions of plain integers (host only, no
// HIP header: tests/test_ctc_plan_cpu.py compiles this file with g++ and compares every decision with a recorded
// table).  capi_ctc.hip validates, plans, lays out, uploads and launches; the launchers of ctc_fused.hip,
// ctc_fusedw.hip, ctc_kernels.hip and ctc_generic.hip turn a plan into a template instantiation and decide nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sctc.h"

namespace sctc {

// per-utterance descriptor, uploaded by the host once per batch
struct CtcUtt {
    int32_t T, U;
    int64_t row0;     // first row (contiguous layout) or rank in the packed minibatch
    int64_t lat_off;  // element offset of this utterance's lattice
    int64_t lab_off;  // first label in the concatenated label array
};

// ctc_fusedw.hip: flag words per utterance; behind the (evenly many) utterances' words, 64 doubles of dump area (stores
// of lanes / frames that have nothing to store)
static constexpr int FUSEDW_SYNC_WORDS = 4;
static inline size_t ctc_fusedw_sync_bytes(int B) { return sizeof(uint32_t) * FUSEDW_SYNC_WORDS * (size_t)((B + 1) & ~1) + 64 * sizeof(double); }

// ---------------------------------------------------------------- the switches ("switches")

struct CtcSwitches {
    int generic = 0;            // SCTC_CTC_GENERIC=1: ctc_generic.hip for every shape
    int lazy = 0;               // SCTC_CTC_LAZY=1: float32 probabilities rescale every 4th frame only (lattice + grad kernels)
    int fused = 1;              // SCTC_CTC_FUSED=0: the lattice + grad kernels instead of the two fused ones (A/B, tests)
    int store = 0;              // SCTC_CTC_STORE=64: float64 rows on the float32 path too (A/B, tests)
    int wide = -1;              // SCTC_CTC_WIDE=0 / 1: never / always the wide fused kernel (-1: by batch size)
    int wide_min_b = -1;        // SCTC_CTC_WIDE_MIN_B: the wide kernel from this many utterances on (-1: 18 / 24, ctc_plan)
    int waves = 0;              // SCTC_CTC_WAVES=1 / 4 / 8: waves per direction of the lattice kernel, 8 of the wide kernel too (diagnostics)
    int helper = -1;            // SCTC_CTC_HELPER=0 / 1: forces the two-wave / six-wave form of the fused kernel (-1: by batch size)
    int helper_max_b = 256;     // SCTC_CTC_HELPER_MAX_B: helper waves up to this many utterances
    int diet_min_b = 1025;      // SCTC_CTC_DIET_MIN_B: the dieted two-wave form from this many utterances on
    int diag = 0;               // SCTC_CTC_DIAG: timing experiments of the fused kernels, results are WRONG (CtcFusedArgs::diag)
};

// The one reader of the environment in the CTC sources; once per call (tests flip switches between calls).
static inline CtcSwitches ctc_switches_from_env()
{
    CtcSwitches s;
    const auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
    s.generic = num("SCTC_CTC_GENERIC", 0) != 0;
    s.lazy = num("SCTC_CTC_LAZY", 0);
    s.fused = num("SCTC_CTC_FUSED", 1) != 0;
    s.store = num("SCTC_CTC_STORE", 0);
    s.wide = num("SCTC_CTC_WIDE", -1);
    const int unset = INT32_MIN, min_b = num("SCTC_CTC_WIDE_MIN_B", unset), helper = num("SCTC_CTC_HELPER", unset);
    if (min_b != unset) s.wide_min_b = min_b > 0 ? min_b : 0;
    s.waves = num("SCTC_CTC_WAVES", 0);
    if (helper != unset) s.helper = helper != 0;
    s.helper_max_b = num("SCTC_CTC_HELPER_MAX_B", s.helper_max_b);
    s.diet_min_b = num("SCTC_CTC_DIET_MIN_B", s.diet_min_b);
    s.diag = num("SCTC_CTC_DIAG", 0);
    return s;
}

// ---------------------------------------------------------------- which instantiations exist

// probability registers per frame and lane: alphabets of up to 64 / 128 / 256 symbols
constexpr int ctc_na(int A) { return A <= 64 ? 1 : (A <= 128 ? 2 : 4); }

// ctc_fused_kernel<RI, ST, K, NA, HELP = true>: helper waves for up to two probability registers per frame; at 8 states
// per lane for alphabets of up to 64 symbols and the 32-bit row store only (the helper's register budget is 256)
constexpr bool ctc_fused_help_exists(int st_bytes, int K, int NA) { return K == 8 ? (NA == 1 && st_bytes == 4) : NA <= 2; }

// ctc_fused_kernel<..., DIET = true>: the two-wave float32 / 32-bit-row kernel of up to 4 states per lane and 64 symbols
// (ctc_fused.hip, FusedDiet)
#ifdef SCTC_FUSED_NO_DIET       // A/B build without it (tools/build_variant.sh, -DSCTC_FUSED_NO_DIET): for ctc_fused.hip AND capi_ctc.hip --
                                // a plan built with the diet asks a ctc_fused.hip built without it for a kernel it lacks: SCTC_ERR_ARG
static constexpr bool CTC_FUSED_DIET_BUILT = false;
#else
static constexpr bool CTC_FUSED_DIET_BUILT = true;
#endif
constexpr bool ctc_fused_diet_exists(int ri_bytes, int st_bytes, int K, int NA, bool help)
{
    return CTC_FUSED_DIET_BUILT && !help && NA == 1 && K <= 4 && ri_bytes == 4 && st_bytes == 4;
}

// ---------------------------------------------------------------- the plan

enum CtcPath {
    CTC_FUSED,      // ctc_fused.hip: both recursions and the gradient in one kernel, one wave per direction, rows of <= 512 states
    CTC_WIDE,       // ctc_fusedw.hip: the same schedule on W = 4 / 8 waves per direction, rows of <= 2048 states
    CTC_LATTICE,    // ctc_kernels.hip: ctc_lattice_kernel + ctc_grad_kernel, rows of <= 2048 states
    CTC_GENERIC,    // ctc_generic.hip: any label length, any alphabet
};

struct CtcShape {
    int B, A, dtype;        // utterances, alphabet, SCTC_F32 | SCTC_F64 (type of probs and grad)
    int max_L, max_T;       // longest label row in lattice states (2U+1), longest utterance in frames
};

struct CtcPlan {
    CtcPath path = CTC_GENERIC;
    int B = 0, A = 0, dtype = SCTC_F32, max_T = 0;
    int K = 0, W = 0;       // states per lane, waves per (utterance, direction); GENERIC: 0, 0
    int lp = 0;             // lattice row stride 64*W*K; GENERIC: round_up(max_L + 1, 64), the width of its scratch rows
    int NA = 0;             // ctc_na(A); GENERIC: unused
    int store_bytes = 8;    // FUSED / WIDE: 4 = the 32-bit row format of ctc_fused.hip (float32 probabilities), 8 = float64 rows
    int lazy = 0;           // LATTICE, float32 probabilities: SCTC_CTC_LAZY
    int help = 0, diet = 0; // FUSED: helper waves (six waves per utterance); the dieted instantiation
    int NB = 0;             // LATTICE: row slices per trip of ctc_grad_kernel
    int diag = 0;           // FUSED / WIDE: CtcFusedArgs::diag
};

// Lattice kernel shape for label rows of up to max_L = 2U+1 <= 2048 states: K states per lane, W waves per
// (utterance, pass).  Up to 256 states one wave holds everything (no cross-wave traffic); longer
// rows are spread over 4 waves so that a frame costs K/4 as many dependent float64 operations, and
// rows of more than 1024 states over 8 waves (two per SIMD): at T = 8000 / U = 800 a frame costs 0.65
// instead of 0.73 us with 4 states per lane instead of 8 (round 3; 16 waves x 2 states: 1.2 us --
// four waves per SIMD meet at the frame's barrier; 8 waves x 2 states for 513..1024 states: 2-4 %
// slower than 4 waves x 4).  Costs and gradients agree to all printed digits
// between the shapes (tests/gpu_ctc_shape.py); the band sum is taken in another order, so the last
// bits of a lattice may differ from one shape to the other.  `force`: SCTC_CTC_WAVES (diagnostics: 1 / 4 / 8).
static inline int ctc_lattice_shape(int max_L, int force, int* waves)
{
    if ((force == 0 && max_L <= 256) || force == 1) {
        *waves = 1;
        for (int k = 2; k <= 32; k *= 2)
            if (max_L <= 64 * k) return k;
        return 0;
    }
    if (force == 8 || (force == 0 && max_L > 1024)) {
        *waves = 8;
        return max_L <= 1024 ? 2 : (max_L <= 2048 ? 4 : 0);
    }
    *waves = 4;
    for (int k = 2; k <= 8; k *= 2)
        if (max_L <= 256 * k) return k;
    return 0;
}

static inline CtcPlan ctc_plan(const CtcShape& s, const CtcSwitches& sw)
{
    const bool f32 = s.dtype == SCTC_F32;
    // label rows of more than 2048 states and alphabets of more than 256 symbols (the reference bounds neither,
    // ctc_fast.pyx:22-32): the generic kernels of ctc_generic.hip
    const bool generic = s.max_L > 2048 || s.A > 256 || sw.generic;
    // the lazy rescaling schedule exists in the lattice + grad kernels only
    const bool lazy = !generic && sw.lazy;
    const bool fused_on = !generic && !lazy && sw.fused;
    // Rows of up to 512 states: both recursions and the gradient in ONE kernel that keeps one packed half lattice
    // per direction (ctc_fused.hip): one wave per direction with 2 / 4 / 8 states per lane (rows of up to 128 / 256 /
    // 512 states: cfg-4's 401 included)
    const int narrow_k = s.max_L <= 128 ? 2 : (s.max_L <= 256 ? 4 : (s.max_L <= 512 ? 8 : 0));
    const bool narrow = fused_on && narrow_k > 0;
    // Rows of 513..2048 states (round 6): the same schedule on W = 4 / 8 waves per direction (ctc_fusedw.hip), from
    // SCTC_CTC_WIDE_MIN_B utterances on (default 18; rows of up to 1024 states, four waves: 24).  Below that the lattice
    // + grad kernels are faster -- their gradient kernel spreads over the CUs the few recursion workgroups leave idle
    // (ms per call, wide / lattice + grad; cfg-5 shape, T = 8000 / U = 800: 8 utterances 5.40 / 4.95, 16: 5.45 / 5.39, 24:
    // 5.48 / 5.82, 128: 6.0 / 15; T = 4000 / U = 511: 16: 2.17 / 2.05, 24: 2.19 / 2.19, 32: 2.22 / 2.28) -- at five times
    // the traffic and ten times the workspace.  SCTC_CTC_WIDE=1 forces it for every row, 0 switches it off.
    const int wide_min_b = sw.wide_min_b >= 0 ? sw.wide_min_b : (s.max_L > 1024 ? 18 : 24);
    const bool wide = fused_on && sw.wide != 0 && (sw.wide == 1 || (!narrow && s.B >= wide_min_b));

    CtcPlan p;
    p.path = generic ? CTC_GENERIC : (wide ? CTC_WIDE : (narrow ? CTC_FUSED : CTC_LATTICE));
    p.B = s.B;
    p.A = s.A;
    p.dtype = s.dtype;
    p.max_T = s.max_T;
    p.NA = ctc_na(s.A);
    // float32 probabilities keep their rows in the 32-bit format of ctc_fused.hip unless SCTC_CTC_STORE=64
    p.store_bytes = (f32 && sw.store != 64) ? 4 : 8;
    p.lazy = f32 && lazy ? sw.lazy : 0;
    p.diag = sw.diag;
    switch (p.path) {
    case CTC_GENERIC:
        p.lp = (s.max_L + 1 + 63) / 64 * 64;
        return p;
    case CTC_WIDE:
        p.W = (s.max_L > 1024 || sw.waves == 8) ? 8 : 4;
        p.K = s.max_L <= 64 * p.W * 2 ? 2 : 4;
        break;
    case CTC_FUSED:
        p.W = 1;
        p.K = narrow_k;
        // Helper waves (six waves per utterance) while the batch leaves SIMDs idle; beyond SCTC_CTC_HELPER_MAX_B
        // utterances (default 256: one six-wave workgroup per CU) the two-wave form keeps more utterances resident
        // (four workgroups per CU; 4096 utterances of the cfg-3 shape: 3.5 ms against 4.5).  SCTC_CTC_HELPER=0 / 1
        // forces one form (A/B, tests) -- where the six-wave form exists.
        p.help = ctc_fused_help_exists(p.store_bytes, p.K, p.NA) && (sw.helper >= 0 ? sw.helper != 0 : s.B <= sw.helper_max_b);
        // From 1025 utterances on the dieted form (three waves per SIMD: 1536 utterances resident instead of 1024;
        // measurements in ctc_fused.hip, FusedDiet)
        p.diet = ctc_fused_diet_exists(f32 ? 4 : 8, p.store_bytes, p.K, p.NA, p.help != 0) && s.B >= sw.diet_min_b;
        break;
    case CTC_LATTICE:
        p.K = ctc_lattice_shape(s.max_L, sw.waves, &p.W);
        break;
    }
    p.lp = 64 * p.W * p.K;
    // (short rows: four slices per trip -- the clamped loads of slices beyond the row are not free: 4096 utterances of
    // 201 states took 7.3 instead of 5.0 ms with sixteen)
    if (p.path == CTC_LATTICE) p.NB = p.lp <= 256 ? 4 : (p.lp <= 512 ? 8 : 16);
    return p;
}

// ---------------------------------------------------------------- the workspace

static inline size_t ctc_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// lattice elements of one utterance: FUSED / WIDE: T packed rows of round_up(2U+1, K) states behind a K-element pad
// (store_bytes each, ONE row store); LATTICE: T rows of lp float64 per direction; GENERIC: rows of its own stride
static inline int64_t ctc_utt_elems(const CtcPlan& p, int T, int U)
{
    const int64_t L = 2 * (int64_t)U + 1;
    if (p.path == CTC_FUSED || p.path == CTC_WIDE) return p.K + (int64_t)T * ((L + p.K - 1) / p.K * p.K);
    if (p.path == CTC_GENERIC) return (int64_t)T * ((L + 1 + 63) / 64 * 64);
    return (int64_t)T * p.lp;
}

// byte offsets of the slices (each rounded up to 256 bytes) and their total
struct CtcLayout {
    int64_t n_labels = 0, lat_elems = 0;
    size_t utts = 0;        // CtcUtt[B]
    size_t labels = 0;      // int32: [n_labels] labels | [n_labels] odd states grouped by label (ctc_grad's per-label sums) | [B][A+1] group offsets
    size_t store = 0, sync = 0;                                 // FUSED / WIDE: the row store; WIDE: ctc_fusedw_sync_bytes(B)
    size_t ll = 0, skip2 = 0, alpha = 0, beta = 0, scratch = 0; // LATTICE / GENERIC: double[2B], int32[2B], double[lat_elems] x 2; GENERIC: double[4 B lp]
    size_t bytes = 0;
};

static inline CtcLayout ctc_layout_slices(CtcPath path, int B, int A, int64_t n_labels, int64_t lat_elems, int lp, int store_bytes)
{
    CtcLayout l;
    l.n_labels = n_labels;
    l.lat_elems = lat_elems;
    size_t at = 0;
    const auto take = [&at](size_t bytes) { const size_t off = at; at += ctc_align256(bytes); return off; };
    l.utts = take(sizeof(CtcUtt) * B);
    l.labels = take(sizeof(int32_t) * (2 * n_labels + (int64_t)B * (A + 1)));
    if (path == CTC_FUSED || path == CTC_WIDE) {
        l.store = take((size_t)store_bytes * lat_elems);
        if (path == CTC_WIDE) l.sync = take(ctc_fusedw_sync_bytes(B));
    } else {
        l.ll = take(sizeof(double) * 2 * B);
        l.skip2 = take(sizeof(int32_t) * 2 * B);
        l.alpha = take(sizeof(double) * lat_elems);
        l.beta = take(sizeof(double) * lat_elems);
        if (path == CTC_GENERIC) l.scratch = take(sizeof(double) * 4 * (size_t)B * lp);
    }
    l.bytes = at;
    return l;
}

// The workspace of one call; `utts` (optional, [B]): T, U, lat_off and lab_off of every descriptor are filled in.
static inline CtcLayout ctc_layout(const CtcPlan& p, const int32_t* T_b, const int32_t* U_b, CtcUtt* utts = nullptr)
{
    const bool packed = p.path == CTC_FUSED || p.path == CTC_WIDE;
    int64_t lat_off = 0, lab_off = 0;
    for (int b = 0; b < p.B; ++b) {
        if (utts) {
            utts[b].T = T_b[b];
            utts[b].U = U_b[b];
            utts[b].lat_off = packed ? lat_off + p.K : lat_off;     // K elements of pad in front (ctc_fused.hip)
            utts[b].lab_off = lab_off;
        }
        lat_off += ctc_utt_elems(p, T_b[b], U_b[b]);
        lab_off += U_b[b];
    }
    return ctc_layout_slices(p.path, p.B, p.A, lab_off, lat_off, p.lp, p.store_bytes);
}

// ---------------------------------------------------------------- kernel names

// The template-ids of the kernels the call launches (one or two), e.g. "ctc_fused_kernel<float, unsigned int, 4, 1, true, false>".
// Returns their number.
static inline int ctc_plan_kernel_name(const CtcPlan& p, char names[2][96])
{
    const char* ri = p.dtype == SCTC_F32 ? "float" : "double";
    const char* st = p.store_bytes == 4 ? "unsigned int" : "double";
    const auto tf = [](int v) { return v ? "true" : "false"; };
    switch (p.path) {
    case CTC_FUSED:
        snprintf(names[0], 96, "ctc_fused_kernel<%s, %s, %d, %d, %s, %s>", ri, st, p.K, p.NA, tf(p.help), tf(p.diet));
        return 1;
    case CTC_WIDE:
        snprintf(names[0], 96, "ctc_fusedw_kernel<%s, %s, %d, %d, %d>", ri, st, p.K, p.NA, p.W);
        return 1;
    case CTC_LATTICE:
        snprintf(names[0], 96, "ctc_lattice_kernel<%s, %d, %d, %d, %s>", ri, p.K, p.NA, p.W, tf(p.lazy));
        snprintf(names[1], 96, "ctc_grad_kernel<%s, %d>", ri, p.NB);
        return 2;
    case CTC_GENERIC:
        snprintf(names[0], 96, "ctc_lattice_generic_kernel<%s>", ri);
        snprintf(names[1], 96, "ctc_grad_generic_kernel<%s>", ri);
        return 2;
    }
    return 0;
}

}  // namespace sctc
