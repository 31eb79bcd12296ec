// Which recurrent kernel a launch gets, and how a minibatch is cut into launches: pure functions of plain
// integers (host only, no HIP header: tests/test_recurrence_plan_cpu.py compiles this file with g++ and compares
// every decision with a recorded table).  recurrent.hip turns a candidate into a kernel pointer and launches it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <initializer_list>

namespace sctc {

// RecArgs.variant / SCTC_REC_VARIANT.  Any other value is an error (launch_recurrent: SCTC_ERR_ARG).
enum RecVariant : int32_t {
    REC_V_AUTO = 0,
    // selection overrides
    REC_V_SLAB = 1,            // the one-slab-per-CU kernel (brnn_recurrent_kernel) at every minibatch size
    REC_V_FALLBACK = 3,        // the non-persistent per-step fallback
    REC_V_S_TO_8 = 43,         // the sentinel / VALU kernel for up to 8 utterances (default: up to 3, then the single-chain flag kernel)
    REC_V_Q_FROM_1 = 44,       // the single-chain flag kernel from 1 utterance (default: from 4)
    REC_V_NO_CUT = 45,         // a minibatch of up to 128 utterances is never cut (default: rec_cut below)
    REC_V_SLAB_LARGE = 47,     // more than 32 utterances on the one-slab-per-CU kernel (default at 1824 / 2048 units: the tiled kernel)
    REC_V_T_SMALL = 50,        // the tiled kernel above 32 utterances at 512 / 1024 units as well (no faster there; tests)
    REC_V_Q_AT_32 = 51,        // 17..32 utterances on the two-chain kernel (default at 1824 / 2048 units, fp32: the tiled kernel, UG = 1)
    // The BPTT launch that the engine runs weight-gradient GEMMs beside (bwd_overlap_plan.h; fp32, 17..32 utterances, 1824 / 2048
    // units -- anywhere else both mean REC_V_AUTO).  Either form claims so much LDS that no GEMM block fits next to its workgroup.
    REC_V_T_HALF = 52,         // the tiled kernel with 32 units x both utterance tiles of a direction per CU: half the grid, Hp / 16 CUs
    REC_V_T_CLAIM = 53,        // the default kernel (UG = 1, Hp / 8 CUs) with the larger LDS claim
    // bit-identical A/Bs that tests use as references
    REC_V_NO_PIPE = 40,        // more than 32 utterances on the one-slab-per-CU kernel without its load / MFMA pipelining
    REC_V_ROW_MAJOR = 46,      // exchange tiles row-major throughout instead of the lane-order layout
    // diagnostics
    REC_V_Q_LINEAR = 2,        // two-chain kernel with the linear (not XCD-grouped) block map
    REC_V_Q_PRIO_DIR = 5, REC_V_Q_PRIO_TILE = 6, REC_V_Q_PRIO_PARITY = 7,  // two-chain kernel, static issue priority by direction / tile / chain parity
    REC_V_T_STALE = 49,        // WRONG RESULTS: the tiled kernel re-reads step 0's exchange rows (timing without fresh data)
};

static inline bool rec_variant_known(int v)
{
    for (int known : {REC_V_AUTO, REC_V_SLAB, REC_V_FALLBACK, REC_V_S_TO_8, REC_V_Q_FROM_1, REC_V_NO_CUT, REC_V_SLAB_LARGE,
                      REC_V_T_SMALL, REC_V_Q_AT_32, REC_V_T_HALF, REC_V_T_CLAIM, REC_V_NO_PIPE, REC_V_ROW_MAJOR, REC_V_Q_LINEAR, REC_V_Q_PRIO_DIR,
                      REC_V_Q_PRIO_TILE, REC_V_Q_PRIO_PARITY, REC_V_T_STALE})
        if (v == known) return true;
    return false;
}

struct RecShape {
    int Hp, B;          // padded layer size; utterances of the launch (rec_cut: of the rest of the minibatch)
    int prec16, transpose;      // "fp16 activations"; BPTT
    int variant;        // RecVariant
    int tcfg, cus;      // SCTC_REC_TCFG (A/B of the tiled kernel's schedule, 0: default); compute units of the device
};

enum RecFamily {
    REC_FAM_Q,          // brnn_recurrent_q_kernel<NCQ, NREG>: flag / MFMA kernel, one or two chains per direction
    REC_FAM_S,          // brnn_recurrent_s_kernel<NK, SB>: sentinel / VALU kernel
    REC_FAM_MH,         // brnn_recurrent_mh_kernel<NCH, BF>: sentinel / MFMA kernel, 16-bit operands
    REC_FAM_T,          // brnn_recurrent_t_kernel<NCQ, NREGF, NT, NBAT, R, PUB, PB, UG[, HALF]>: tiled over units x utterances
    REC_FAM_SLAB,       // brnn_recurrent_kernel<NTW, NCHH, PIPE>: one 16-unit slab per CU
    REC_FAM_FALLBACK,   // brnn_recurrent_step_kernel, one launch per time step: always the plan's last candidate
};

struct RecCandidate {
    RecFamily family;
    int ntarg, targ[9];     // template arguments, in the kernel's order
    int grid;
    size_t lds;             // dynamic LDS bytes
    int per_cu;             // workgroups of this kernel that share a CU
    int fill;               // bytes per exchange element to fill with the 0xFF sentinel before the launch (0: none)
    int linear_map;         // RecArgs.linear_map
    int variant;            // RecArgs.variant as the kernel sees it
};
static constexpr int REC_MAX_CANDIDATES = 6;    // at most two of Q / S / MH / T (REC_V_T_HALF: three), then SLAB, then the fallback (one spare)

// The per-layer-size facts.
// <weight fragments in registers, batches per phase, ring depth, publish batch, batch in front of which the next
// phase's flags are checked> of brnn_recurrent_t_kernel; nbat == 0: no such instantiation
struct RecTForm { int nregf, nbat, r, pub, pb; };
constexpr RecTForm rec_t84(int nregf) { return {nregf, 8, 4, 1, 5}; }
constexpr RecTForm rec_t63(int nregf) { return {nregf, 6, 3, 1, 4}; }
constexpr RecTForm rec_t82(int nregf) { return {nregf, 8, 2, 1, 7}; }      // ring of two: one batch of lookahead (slower; shows what the ring hides)
constexpr RecTForm rec_t42(int pub) { return {0, 4, 2, pub, 3}; }

struct RecSize {
    int Hp;
    int ncq, nreg;          // Q: chunks per wave, of them in registers (keeps the slab's LDS share at <= 76 KiB per workgroup)
    int nk;                 // S (NK) and SLAB (NCHH): Hp / 32
    int nch;                // MH: ceil(nk / 4)
    bool t_default;         // above 32 utterances the tiled kernel is the default (else only with REC_V_T_SMALL: no faster)
    // T by SCTC_REC_TCFG 0..3 (A/B of the schedule; 3 = UG 1 with the weight slab in LDS instead of the accumulation registers):
    RecTForm t_ug1[4];      // UG = 1: 17..32 utterances
    RecTForm t_one[4];      // one utterance tile per sub-chain: 33..64
    RecTForm t_two[4];      // two: 65..128 (1824 units: 8, 4 would need 128 ring registers, 28 of them parked in the other file)
};
static constexpr RecSize REC_SIZES[] = {
    {512, 8, 0, 16, 4, false, {}, {rec_t42(0), rec_t42(0), rec_t42(0), rec_t42(0)}, {rec_t42(0), rec_t42(0), rec_t42(0), rec_t42(0)}},
    {1024, 16, 0, 32, 8, false, {}, {rec_t42(1), rec_t42(1), rec_t42(1), rec_t42(1)}, {rec_t42(1), rec_t42(1), rec_t42(1), rec_t42(1)}},
    {1824, 29, 10, 57, 15, true, {rec_t84(29), rec_t63(29), rec_t84(29), rec_t84(0)},
     {rec_t84(25), rec_t63(25), rec_t82(25), rec_t84(25)}, {rec_t63(25), rec_t84(25), rec_t82(25), rec_t63(25)}},
    {2048, 32, 13, 64, 16, true, {rec_t84(32), rec_t63(32), rec_t84(32), rec_t84(0)},
     {rec_t84(31), rec_t63(31), rec_t84(31), rec_t84(31)}, {rec_t84(31), rec_t63(31), rec_t84(31), rec_t84(31)}},
};
static inline const RecSize* rec_size(int Hp)
{
    for (const RecSize& r : REC_SIZES) if (r.Hp == Hp) return &r;
    return nullptr;
}

// dynamic LDS of each family
static constexpr size_t REC_LDS_MAX = 160 * 1024, REC_F4 = 16;    // LDS of a CU; sizeof(float4)
// A workgroup that claims this much leaves less than any fp32 GEMM block needs (the smallest takes 25 KiB, gemm_plan.h;
// tests/test_bwd_overlap_plan_cpu.py): GEMM blocks of a concurrent launch go to the CUs this grid does not occupy.
static constexpr size_t REC_LDS_EXCLUDES_GEMM = REC_LDS_MAX - 16 * 1024;
// the LDS share of the wave-private weight fragments + the K-quarter partial sums of three waves
static inline size_t rec_lds_q(const RecSize& r) { return REC_F4 * ((size_t)4 * (r.ncq - r.nreg) * 64 + 3 * 64); }
static inline size_t rec_lds_s(int Hp, int sb) { return sizeof(float) * 2 * sb * Hp; }
static inline size_t rec_lds_mh(int Hp) { return (((size_t)16 * (Hp + 8) * 2 + 15) / 16) * 16 + 3 * 64 * REC_F4; }
// NLDSF = UG * NCQ - NREGF fragments per wave, [2 phase parities][NC = UG * NT results][3 other waves] partial sums, flag words
static inline size_t rec_lds_t(const RecSize& r, const RecTForm& f, int nt, int ug) { return REC_F4 * 64 * ((size_t)4 * (ug * r.ncq - f.nregf) + 2 * 3 * (ug * nt)) + (16 * 8 + 8 * 32) * sizeof(unsigned); }
static inline size_t rec_lds_slab(int Hp, int ntw) { return REC_F4 * ((size_t)(Hp / 16) * 64 + 2 * ntw * 64); }

// Is the tiled kernel (two sub-chains per CU) what more than 32 utterances run on?  rec_plan and rec_cut both ask here.
static inline bool rec_tiled_large(const RecShape& s)
{
    const RecSize* r = rec_size(s.Hp);
    return r && s.variant != REC_V_SLAB && s.variant != REC_V_NO_PIPE && s.variant != REC_V_SLAB_LARGE &&
           4 * (s.Hp / 32) <= s.cus && (r->t_default || s.variant == REC_V_T_SMALL);
}

static inline RecCandidate rec_candidate(const RecShape& s, RecFamily family, std::initializer_list<int> targ, int grid,
                                         size_t lds, int per_cu, int fill)
{
    RecCandidate c = {family, (int)targ.size(), {}, grid, lds, per_cu, fill, 0, s.variant};
    std::copy(targ.begin(), targ.end(), c.targ);
    return c;
}
static inline RecCandidate rec_candidate_t(const RecShape& s, const RecSize& r, const RecTForm& f, int nt, int ug, size_t lds_min)
{
    return rec_candidate(s, REC_FAM_T, {r.ncq, f.nregf, nt, f.nbat, f.r, f.pub, f.pb, ug}, 2 * ug * (s.Hp / (16 * ug)),
                         std::max(rec_lds_t(r, f, nt, ug), lds_min), 1, 0);
}

// The candidates of one launch (s.B <= 128 utterances) in the order they are tried; the launcher skips a candidate the
// device cannot co-reside.  Returns their number, or -1 for a variant that does not exist.
static inline int rec_plan(const RecShape& s_in, RecCandidate out[REC_MAX_CANDIDATES])
{
    if (!rec_variant_known(s_in.variant)) return -1;
    // the two overlap forms are the default plan with one candidate put in front (half grid) or its LDS claim raised
    RecShape s = s_in;
    const bool t_half = s_in.variant == REC_V_T_HALF, t_claim = s_in.variant == REC_V_T_CLAIM;
    if (t_half || t_claim) s.variant = REC_V_AUTO;
    const int nwg = s.Hp / 16, ntiles = (s.B + 15) / 16, v = s.variant, B = s.B, sb = B <= 4 ? 4 : 8;
    const RecSize* r = rec_size(s.Hp);
    const int tcfg = s.tcfg >= 0 && s.tcfg <= 3 ? s.tcfg : 0;
    // a persistent grid has at least one workgroup per 16 units and direction: if that does not fit, only the fallback is left
    const bool persistent = v != REC_V_FALLBACK && 2 * nwg <= s.cus;
    int n = 0;
    // (the measurements behind every choice: DESIGN.md 4.2)  4..16 utterances (16-bit operands: up to 5) are ONE 16-utterance chain on
    // the flag kernel of the 17..32 case; from 4 on it beats the sentinel / VALU kernel below, whose step grows with every utterance
    if (persistent && r && (!s.prec16 || B <= 5) && (B >= 4 || v == REC_V_Q_FROM_1) && B <= 16 && v != REC_V_SLAB && v != REC_V_S_TO_8) {
        RecCandidate c = rec_candidate(s, REC_FAM_Q, {r->ncq, r->nreg}, 2 * nwg, rec_lds_q(*r), 2, 0);
        c.linear_map = 1;   // linear block -> (chain, producer) map: chain = direction, tile 0 only (variant keeps its A/B meaning)
        if (v == REC_V_Q_FROM_1) c.variant = REC_V_AUTO;
        out[n++] = c;
    }
    // <= 239 VGPRs and 58 KiB of LDS (1..4 utterances at H = 1824): TWO of these workgroups fit a CU, so the grids of two
    // streams (one utterance per stream) can be co-resident -- the in-process gate counts this launch as half the device
    if (persistent && r && (B <= 5 || (B <= 8 && v == REC_V_S_TO_8)) && v != REC_V_SLAB)
        out[n++] = rec_candidate(s, REC_FAM_S, {r->nk, sb}, 2 * nwg, rec_lds_s(s.Hp, sb), 2, 4);
    // "fp16 activations": 16-bit state exchange and weights (float16 forward, bfloat16 BPTT)
    if (persistent && r && s.prec16 && B > 5 && B <= 16 && v != REC_V_SLAB && rec_lds_mh(s.Hp) <= REC_LDS_MAX)
        out[n++] = rec_candidate(s, REC_FAM_MH, {r->nch, s.transpose != 0}, 2 * nwg, rec_lds_mh(s.Hp), 1, 2);
    // 17..32 utterances, fp32, H = 1824 / 2048: the tiled kernel with 16 units x both utterance tiles of a direction per CU.  With its
    // slab in registers a second workgroup would fit a CU: more than half of the LDS is claimed (the co-residency check counts CUs)
    // REC_V_T_HALF: the 33..64 form (32 units, two alternating sub-chains) with combo = direction, tile = sub-chain, on
    // 2 * Hp / 32 CUs; its slab takes 144 KiB of LDS by itself.  The default schedule only (one instantiation per layer size).
    if (t_half && persistent && r && r->t_default && ntiles == 2 && !s.prec16) {
        RecCandidate c = rec_candidate_t(s, *r, r->t_one[0], 1, 2, REC_LDS_EXCLUDES_GEMM);
        c.targ[c.ntarg++] = 1;      // HALF
        c.grid = 2 * (s.Hp / 32);
        out[n++] = c;
    }
    if (persistent && r && r->t_ug1[tcfg].nbat && ntiles == 2 && !s.prec16 && (v == REC_V_AUTO || v == REC_V_ROW_MAJOR || v == REC_V_T_STALE))
        out[n++] = rec_candidate_t(s, *r, r->t_ug1[tcfg], 1, 1, t_claim ? REC_LDS_EXCLUDES_GEMM : (size_t)81 * 1024);
    // two chains per CU
    if (persistent && r && ntiles == 2 && v != REC_V_SLAB && 4 * nwg <= 2 * s.cus)
        out[n++] = rec_candidate(s, REC_FAM_Q, {r->ncq, r->nreg}, 4 * nwg, rec_lds_q(*r), 2, 0);
    // 33..128 utterances: 32 units x half the utterance tiles per CU, two alternating sub-chains
    if (persistent && ntiles > 2 && rec_tiled_large(s))
        out[n++] = ntiles <= 4 ? rec_candidate_t(s, *r, r->t_one[tcfg], 1, 2, 0) : rec_candidate_t(s, *r, r->t_two[tcfg], 2, 2, 0);
    // one slab per CU; PIPE measured slower at two utterance tiles per wave (profiles/r05_recurrence_large.md), NCHH = 0: any layer size
    const int ntw = ntiles <= 2 ? 1 : (ntiles <= 4 ? 2 : 4);
    if (persistent && rec_lds_slab(s.Hp, ntw) <= REC_LDS_MAX)
        out[n++] = rec_candidate(s, REC_FAM_SLAB, {ntw, r ? r->nk : 0, ntw == 4 && r && v != REC_V_NO_PIPE}, 2 * nwg,
                                 rec_lds_slab(s.Hp, ntw), 1, 0);
    out[n++] = rec_candidate(s, REC_FAM_FALLBACK, {}, 0, 0, 0, 0);
    return n;
}

// How many of the s.B utterances that are left (sorted by length) the next launch takes.  Utterances are independent and a
// later launch covers only as many steps as ITS longest utterance has (tools/rec_tiled_sweep.sh): with the
// tiled kernel 65..96 run as 64 + the rest (one launch of the two-tile form multiplies its empty tile slots), without it
// 33..48 as 32 + the rest and 65..80 as 64 + the rest.  Only the default and REC_V_T_SMALL with fp32 operands cut at all.
static inline int rec_cut(const RecShape& s)
{
    const int nb = s.B < 128 ? s.B : 128;
    const bool cuts = (s.variant == REC_V_AUTO || s.variant == REC_V_T_SMALL) && !s.prec16;
    if (cuts && rec_tiled_large(s)) return nb > 64 && nb <= 96 ? 64 : nb;
    if (cuts && s.variant == REC_V_AUTO) return nb > 32 && nb <= 48 ? 32 : (nb > 64 && nb <= 80 ? 64 : nb);
    return nb;
}

// the kernel's template-id, e.g. "brnn_recurrent_q_kernel<29, 10>"
static inline void rec_candidate_name(const RecCandidate& c, char* buf, size_t len)
{
    static const char* const NAMES[] = {"brnn_recurrent_q_kernel", "brnn_recurrent_s_kernel", "brnn_recurrent_mh_kernel",
                                        "brnn_recurrent_t_kernel", "brnn_recurrent_kernel", "brnn_recurrent_step_kernel"};
    size_t at = snprintf(buf, len, "%s", NAMES[c.family]);
    for (int i = 0; i < c.ntarg && at < len; ++i) {
        const bool flag = (c.family == REC_FAM_MH && i == 1) || (c.family == REC_FAM_SLAB && i == 2);    // BF, PIPE
        if (flag) at += snprintf(buf + at, len - at, "%s%s", i ? ", " : "<", c.targ[i] ? "true" : "false");
        else at += snprintf(buf + at, len - at, "%s%d", i ? ", " : "<", c.targ[i]);
    }
    if (c.ntarg && at < len) snprintf(buf + at, len - at, ">");
}

}  // namespace sctc
