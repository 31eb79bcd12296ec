// CTC forward-backward, "meet in the middle" for LONG label rows (513..2048 lattice states; BASELINE configs[4]:
// T = 8000, U = 800 -> 1601 states): the device counterpart of ctc_fast/ctc-loss/ctc_fast.pyx:13-152 where one
// wave per direction (ctc_fused.hip) no longer holds a row.  Round 6, VERDICT r05 #3.
//
// Rounds 1-5 ran ctc_lattice_kernel + ctc_grad_kernel there: both lattices stored in float64 over a 2048-wide row
// and read back by a third kernel -- 2 x 2.1 GB per cfg-5 step of 8 utterances for 17 MB of algorithmic bytes.  Here:
//
//   * one workgroup per (utterance, direction), W = 4 / 8 waves, K = 2 / 4 states per lane, exactly the
//     recursion of ctc_lattice_kernel<.., W> (state s in global lane s / K, neighbours by DPP, the two cross-wave
//     couplings of a frame -- band sum, boundary state -- through LDS behind ONE barrier per frame);
//   * phase 0: alpha walks t = 0 .. Ta-1 (Ta = T/2), beta walks t = T-1 .. Ta, each STORES its normalised rows,
//     packed to round_up(2U+1, K) states, in the 32-bit format of ctc_store.h on float32 probabilities;
//   * the two workgroups of an utterance meet ONCE (agent-scope release / acquire around a flag word each; they
//     are neighbours in dispatch order, so the partner is resident or the next to become so; bounded spin);
//   * phase 1: alpha walks on to T-1 and multiplies its row, still in registers, with beta's stored row of that
//     frame (beta likewise against alpha's rows): alpha*beta (:117-119) goes to LDS, a row of K*64*W doubles per
//     frame -- NOTHING else happens inside the frame (decode, multiply, one LDS write: the recursion waves are
//     issue-bound, two to a SIMD; the first version formed each lane's share of absum in the frame, three
//     reciprocals and eight fused multiply-adds per lane, and a phase-1 frame cost 1.03 us against 0.57).  Behind
//     every block of PF frames the waves share out the block's frames, one wave per frame: lane k walks label k's
//     host-built list of states (:120-131; its first entries live in registers) for the label sum AND the label's
//     share of absum (:125-136, a product with 1/y[k] per STATE like the reference divides per state), all lanes
//     sum the blank states likewise, then the gradient row (:138-145).  No helper waves, no second kernel; a
//     lattice element is written at most once and read at most once.
//   * skip (a zero band sum, :45 / :75) in either direction takes back every gradient row: the two workgroups
//     exchange their verdicts once more at the end.
//
// Where it is used (ctc_plan, ctc_plan.h): from 18 utterances on (24 for rows of up to 1024 states) -- below that the
// lattice + grad pair is faster, because its gradient kernel runs on the CUs a few recursion workgroups leave idle, while
// here the gradient rows cost the recursion waves their own issue slots (cfg-5 shape: 8 utterances 5.40 against 4.95 ms,
// 24: 5.48 / 5.82, 128: 6.0 / 15); a fifth of the HBM traffic and a tenth of the workspace at every size.
//
// Summation order: as in ctc_fused.hip fixed trees / fixed list order (bit-reproducible run to run, last-bit
// differences against the reference's ascending-state loop; the float64 golden vectors hold at 1e-11 / 1e-9).
//
// From ctc_dev.h: the reciprocals, the row gather / broadcast, the clamped row load and the block's row indices, the
// cross-wave band sum with its boundary state (CrossWave), the LDS-only
// barrier, the lane's sum tree and llForward's running product (LogProduct).
#include <mutex>
#include <type_traits>

#include "common.h"
#include "ctc_dev.h"
#include "ctc_kernels.h"
#include "ctc_store.h"

namespace sctc {

// FUSEDW_SYNC_WORDS (ctc_plan.h) sync words per utterance, zeroed by the launcher: [0..1] phase 0 finished (1 + skip) per
// direction, [2..3] all done

template <typename RI, typename ST, int K, int NA, int W>
__global__ __launch_bounds__(64 * W) void ctc_fusedw_kernel(CtcFusedArgs<RI> p, int B)
{
    using R = double;
    static_assert(K == 2 || K == 4, "2 or 4 states per lane");
    static_assert(W == 4 || W == 8, "4 or 8 waves per direction");
    constexpr int KH = K / 2;
    constexpr int NT = 64 * W;                               // global lanes of a direction
    constexpr int PF = NA * (int)sizeof(RI) >= 16 ? 4 : 8;   // phase 1: frames per block (prefetch depth, frames finished together)
    // phase 0 has no partner rows and no lists in flight: longer blocks there (gfx950 counts loads and stores in one
    // in-order counter, so a block's prefetch also waits for the rows stored before it: once per block)
    constexpr int PF0 = NA * (int)sizeof(RI) >= 8 ? PF : 16;
    constexpr int NST = NT * K;                              // states a direction's lanes hold (> 2U+1: state NST-1 never exists)
    constexpr int NLB = NST / 2;                             // an LDS row of alpha*beta: [NLB blank states][NLB label states]
    constexpr int ZROW = NST - 1;                            // row index of state NST-1, which never exists: its product is
                                                             // always +0 -- the pad entry of the lists
    constexpr int NREGE = NA == 1 ? 40 : (NA == 2 ? 16 : 8); // list entries of a label kept in registers (32-40 registers in all)
    constexpr int REPS = PF > W ? PF / W : 1;                // frames of a block per wave
    using BlkU = RowBlockU<ST, K>;
    using BlkA = RowBlockA<ST, K>;

    __shared__ __attribute__((aligned(16))) typename CrossWave<W>::Slots xw;
    __shared__ int32_t sh_word;
    extern __shared__ __attribute__((aligned(16))) double dyn_s[];
    double* const ab_s = dyn_s;                                               // [PF][NST] alpha*beta of a block's frames, by state
    int32_t* const ord_st = reinterpret_cast<int32_t*>(ab_s + PF * NST);      // [NT*KH] label states (row index, my order) grouped by label
    int32_t* const lstart = ord_st + NT * KH;                                 // [A + 1]

    // block -> (utterance, direction): the two workgroups of an utterance are blocks i and i + 8 -- the same XCD (block
    // i runs on XCD i % 8: the partner's rows may still be in the L2 they were written through) and 8 apart in dispatch
    // order (at most 8 resident workgroups can be waiting for a partner that is not resident yet; every other one
    // finishes and makes room).  Placement only affects speed.
    const int b = ((int)blockIdx.x >> 4) * 8 + ((int)blockIdx.x & 7);
    const int dir = ((int)blockIdx.x >> 3) & 1;          // 0: alpha, 1: beta (== alpha of the reversed problem)
    if (b >= B) return;
    const int lane = threadIdx.x & 63, gl = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const CtcUtt u = p.utts[b];
    const int T = u.T, U = u.U, L = 2 * U + 1;
    const int stride = (L + K - 1) / K * K;
    const int Ta = T / 2, Tb = T - Ta;
    const int Tst = dir ? Tb : Ta;      // my stored rows: tau in [0, Tst)
    ST* mine = reinterpret_cast<ST*>(p.store) + u.lat_off + (dir ? (int64_t)Ta * stride : 0);
    const ST* other = reinterpret_cast<const ST*>(p.store) + u.lat_off + (dir ? 0 : (int64_t)Ta * stride);
    uint32_t* sync = p.sync + (size_t)FUSEDW_SYNC_WORDS * b;
    RI* const dump = reinterpret_cast<RI*>(p.sync + (size_t)FUSEDW_SYNC_WORDS * ((B + 1) & ~1));   // 64 elements nobody reads
    const int32_t* seq = p.labels + u.lab_off;
    const int blank = p.blank;
    const int A = p.A;
    const RI* probs = p.probs;
    RI* grad = p.grad;
    const int64_t ld = p.ld;

    // ---- per-lane constants: labels of my odd states, skip-transition permission (the same in all three kernels)
    int lab[KH];
    bool allow[KH], valid_lab[KH], valid_blk[KH];
    R allowf[KH];
#pragma unroll
    for (int jj = 0; jj < KH; ++jj) {
        const int idx = KH * gl + jj;
        const bool ok = idx < U;
        const int i0 = ok ? (dir ? U - 1 - idx : idx) : 0;
        lab[jj] = seq[i0];
        int prev = blank;
        if (ok && idx >= 1) prev = seq[dir ? U - idx : idx - 1];
        allow[jj] = ok && idx >= 1 && lab[jj] != prev;   // ctc_fast.pyx:64-68 / :103-107
        allowf[jj] = allow[jj] ? (R)1 : (R)0;
        valid_lab[jj] = ok;
        valid_blk[jj] = idx <= U;
    }
    const bool store_lane = K * gl < stride;
    const int other_off = max(L - K * (gl + 1), -K);     // my block of the other direction's (mirrored) row

    // ---- gradient side: lane k (+64q) of EVERY wave owns label k's list of states, in MY direction's order.  The lists
    // go to LDS now; a lane's first NREGE entries are turned into registers right before phase 1 (load_lists): as LDS
    // pointers into the wave's OWN frame row of a block (a wave always finishes the same frames of a block: w, w + W),
    // so a list entry costs its read and the two operations on the value
    {
        const int32_t* start = p.label_start + (int64_t)b * (A + 1);
        const int32_t* byl = p.by_label + u.lab_off;
        for (int j = gl; j < U; j += NT) {
            const int i = byl[j] >> 1;                    // by_label holds states 2i+1 (alpha's order)
            ord_st[j] = NLB + (dir ? U - 1 - i : i);      // index into an LDS row of products
        }
        for (int k = gl; k <= A; k += NT) lstart[k] = start[k];
        __syncthreads();
    }
    const double* lp[NA][NREGE];
    int llen[NA], lj0[NA];
    int maxlen = 0;
    auto load_lists = [&]() {
        const double* mine_row = ab_s + (wave & (PF - 1)) * NST;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int k = lane + 64 * q;
            const int j0 = k < A ? lstart[k] : 0, j1 = k < A ? lstart[k + 1] : 0;
            lj0[q] = j0;
            llen[q] = j1 - j0;
            maxlen = max(maxlen, llen[q]);
#pragma unroll
            for (int n = 0; n < NREGE; ++n) lp[q][n] = mine_row + (n < llen[q] ? ord_st[j0 + n] : ZROW);
        }
        maxlen = wave_max(maxlen);
    };

    // the kernel's context bound to the shared device code (ctc_dev.h); no load or store of the frame loops under a branch
    auto load_row = [&](int64_t row, RI (&dst)[NA]) { load_row_clamped(probs, ld, A, lane, row, dst); };
    auto block_rows = [&](int tau0) -> int { return sctc::block_rows(p.rowbase, T, dir, lane, tau0); };
    auto gather = [&](const RI (&y)[NA], int k) -> R { return (R)row_gather(y, k); };   // probs.astype(np.float64), brnnet.py:175
    auto bcast = [&](const RI (&y)[NA], int k) -> R { return (R)row_bcast(y, k); };
    // the other direction's row of MY frame tau: its own time index is T-1-tau, its state order mine mirrored
    auto load_other = [&](int tau, BlkU& dst) {
        const int taup = T - 1 - min(tau, T - 1);
        // (a lane beyond the row reads the K elements in front of it -- finite values that meet zeros, see products)
        dst = *reinterpret_cast<const BlkU*>(other + (int64_t)taup * stride + other_off);
    };
    // (forwarding lambdas on purpose: with the shared functions called directly at the call sites the compiler ordered
    // the floating-point instructions of 19 of this file's 36 kernels differently)
    auto recip = [&](R c) -> R { return ctc_recip(c); };
    auto recip_or_zero = [&](R y) -> R { return ctc_recip_or_zero<RI>(y); };
    auto local_sum = [&](const R (&n)[K]) -> R { return sum_tree(n); };

    R a[K];
#pragma unroll
    for (int j = 0; j < K; ++j) a[j] = (R)0;
    CrossWave<W> cw;   // band sums over the W waves and the previous wave's boundary state: ONE barrier per frame
    R rprev = (R)1;    // factor the previous frame's row was scaled with
    constexpr int NO_BAD = 0x7fffffff;
    int first_bad = NO_BAD;
    int skip = 0;
    LogProduct llf;    // llForward; frames from the first zero band sum on do not count
    auto ll_account = [&](R c) { llf.account(first_bad == NO_BAD ? c : (R)1); };
    const bool empty_band = (L >= 2 * T + 2) && T > 1;
    auto block_sum = [&](R loc, R last_unnorm, int tau) -> R { return cw.sum(xw, loc, last_unnorm, tau, lane, wave); };

    // one frame of the recursion; FAST: the band starts at state 0 (no band tests)
    auto step = [&](auto fast_tag, int tau, R yb, const R (&yl)[KH]) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const R prev_last = cw.shift_in(a[K - 1], rprev, lane, wave);
        R n[K];
        if constexpr (FAST) {
#pragma unroll
            for (int jj = 0; jj < KH; ++jj) {
                const R below = jj == 0 ? prev_last : a[2 * jj - 1];
                n[2 * jj] = (a[2 * jj] + below) * yb;
                n[2 * jj + 1] = fma(below, allowf[jj], a[2 * jj + 1] + a[2 * jj]) * yl[jj];
            }
        } else {
            const int rem = 2 * (T - tau);           // lower band limit, ctc_fast.pyx:49-53
            const int start = L <= rem ? 0 : L - rem;
#pragma unroll
            for (int jj = 0; jj < KH; ++jj) {
                const R below = jj == 0 ? prev_last : a[2 * jj - 1];
                const int sb = K * gl + 2 * jj;
                const R vb = (a[2 * jj] + below) * yb;                 // :58-62
                n[2 * jj] = (valid_blk[jj] && sb >= start) ? vb : (R)0;
                R in = a[2 * jj + 1] + a[2 * jj];                      // :63-68
                if (allow[jj]) in += below;
                const R vl = in * yl[jj];
                n[2 * jj + 1] = (valid_lab[jj] && sb + 1 >= start) ? vl : (R)0;
            }
        }
        const R c = block_sum(local_sum(n), n[K - 1], tau);
        R r;
        if constexpr (FAST) {
            first_bad = (c == (R)0 && first_bad == NO_BAD) ? tau : first_bad;   // ZeroDivisionError at :75
            r = recip(c);
        } else {
            first_bad = (c == (R)0 && !empty_band && first_bad == NO_BAD) ? tau : first_bad;
            r = empty_band ? (R)1 : recip(c);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) a[j] = n[j] * r;
        rprev = r;
        if constexpr (FAST) ll_account(c);
        else ll_account(empty_band ? (R)1 : c);
    };
    // phase 1, inside the frame: alpha*beta of my states against the other direction's stored row, to the frame's LDS
    // row.  No mask: a state beyond the label row is exactly 0.0 in my registers and what the mirrored block holds
    // there -- the tail of the row stored before, or the pad in front of the first one, which alpha's workgroup zeroes --
    // is finite.
    auto products = [&](int slot, const BlkU& ob) {
        R ab[K];
#pragma unroll
        for (int j = 0; j < K; ++j) ab[j] = a[j] * Store<ST>::dec(ob.v[K - 1 - j]);      // :119
        double* dst = ab_s + slot * NST + KH * gl;
        if constexpr (K == 4) {
            *reinterpret_cast<double2*>(dst) = make_double2(ab[0], ab[2]);
            *reinterpret_cast<double2*>(dst + NLB) = make_double2(ab[1], ab[3]);
        } else {
            dst[0] = ab[0];
            dst[NLB] = ab[1];
        }
    };
    // phase 1, behind a block's frames (and a barrier): ONE frame's sums and gradient row, by one wave
    auto grad_frame = [&](auto rep_tag, int slot, int64_t row, bool frame_valid, const RI (&yc)[NA]) {
        constexpr int ROFF = decltype(rep_tag)::value * W * NST;     // my second frame of a block lies W rows on
        const double* ls = ab_s + slot * NST;
        // This runs between two blocks of frames with every wave waiting for the slowest: it is written for LATENCY.  All
        // of a pass's LDS reads are issued before the first value is used, every sum runs in four independent
        // accumulators (a fixed order all the same), the next group of list entries is in flight while one is summed.
        // blank states (even): the blank sum (:122-124) and their share of absum (:125-126), a product per state
        constexpr int NB = NLB / 64;                 // blank states per lane (an even number), two to a read
        R bv[NB];
#pragma unroll
        for (int m = 0; m < NB; m += 2) {
            const double2 v2 = *reinterpret_cast<const double2*>(ls + 2 * (lane + 32 * m));
            bv[m] = v2.x;
            bv[m + 1] = v2.y;
        }
        R lv[2][8];
#pragma unroll
        for (int n = 0; n < 8; ++n) lv[0][n] = lp[0][n][ROFF];
        const R rb = recip_or_zero(bcast(yc, blank));
        R z4[4], e4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            e4[i] = bv[i];
            z4[i] = bv[i] * rb;
        }
#pragma unroll
        for (int m = 4; m < NB; ++m) {
            e4[m & 3] += bv[m];
            z4[m & 3] = fma(bv[m], rb, z4[m & 3]);
        }
        const R e = (e4[0] + e4[1]) + (e4[2] + e4[3]);
        R g[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const R rk = recip_or_zero((R)yc[q]);    // 1 / y[k]: my own symbol
            R g4[4] = {(R)0, (R)0, (R)0, (R)0};
#pragma unroll
            for (int n0 = 0; n0 < NREGE; n0 += 8) {
                const int cur = (q * (NREGE / 8) + (n0 >> 3)) & 1;     // (compile-time: both loops are unrolled)
                if (n0 + 8 < NREGE) {                 // the next group's reads (pads read the always-zero state)
#pragma unroll
                    for (int n = 0; n < 8; ++n) lv[cur ^ 1][n] = lp[q][n0 + 8 + n][ROFF];
                } else if (q + 1 < NA) {
#pragma unroll
                    for (int n = 0; n < 8; ++n) lv[cur ^ 1][n] = lp[q + 1 < NA ? q + 1 : q][n][ROFF];
                }
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    g4[n & 3] += lv[cur][n];                        // :127-131
                    z4[n & 3] = fma(lv[cur][n], rk, z4[n & 3]);     // :130-131
                }
            }
            for (int n = NREGE; n < maxlen; n += 4) {   // lists longer than the registers hold: from LDS, four per trip
                int st[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) st[i] = n + i < llen[q] ? ord_st[lj0[q] + n + i] : ZROW;
                R v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = ls[st[i]];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    g4[i] += v[i];
                    z4[i] = fma(v[i], rk, z4[i]);
                }
            }
            g[q] = (g4[0] + g4[1]) + (g4[2] + g4[3]);
        }
        const R z = (z4[0] + z4[1]) + (z4[2] + z4[3]);
        const R Z = wave_sum(z);                     // absum[t], :133-136
        const R gb = wave_sum(e);
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int k = lane + 64 * q;
            const R gk = k == blank ? g[q] + gb : g[q];
            const R y = (R)yc[q];
            const R tmp = y * Z;                                         // :141
            const RI out = (RI)(tmp > (R)0 ? y - gk / tmp : y);          // :142-145 (cast: brnnet.py:188)
            RI* dst = (k < A && frame_valid) ? grad + row * ld + k : dump + lane;
            *dst = out;
        }
    };
    // the frames of a finished block are shared out: wave w takes frames w, w + W, ... (their probabilities were
    // fetched with the block's prefetch: yg[rep] = frame w + rep * W)
    auto grad_block = [&](int tb, int t_end, int rows, const RI (&yg)[REPS][NA]) {
        lds_barrier();         // every wave's products of the block's last frame are in LDS
#pragma unroll
        for (int rep = 0; rep < REPS; ++rep) {
            const int i = (wave + rep * W) & (PF - 1);           // uniform
            const bool valid = wave + rep * W < PF && tb + i < t_end;   // (PF < W: the upper waves work for the dump)
            const int64_t row = (int64_t)__builtin_amdgcn_readlane(rows, i) + u.row0;
            if (rep == 0) grad_frame(std::integral_constant<int, 0>(), i, row, valid, yg[rep]);
            else grad_frame(std::integral_constant<int, 1>(), i, row, valid, yg[rep]);
        }
        // the next block's products reach the LDS rows behind that block's first band-sum barrier, which no wave
        // passes before it is done here
    };

    // phase 0: my row of frame tau to the store, EVERY lane (no branch inside a block of frames): a lane beyond the row
    // holds zeros and writes them to the pad in front of the utterance's first row, which must be zero anyway (products)
    ST* const row_base = store_lane ? mine + K * gl : reinterpret_cast<ST*>(p.store) + u.lat_off - K;
    const int64_t row_step = store_lane ? stride : 0;
    auto store_row = [&](int tau) {
        BlkA blk;
#pragma unroll
        for (int j = 0; j < K; ++j) blk.v[j] = Store<ST>::enc(a[j]);
        *reinterpret_cast<BlkA*>(row_base + (int64_t)tau * row_step) = blk;
    };

    // ---- frames [t_begin, t_end) of my direction; PH 0: store the rows, PH 1: form the gradient
    auto run = [&](auto ph_tag, int t_begin, int t_end) {
        constexpr int PH = decltype(ph_tag)::value;
        constexpr int PFr = PH ? PF : PF0;     // frames per block of this phase
        if (skip || t_begin >= t_end) return;
        RI ycur[PFr][NA];
        BlkU ocur[PH ? PFr : 1];
        RI ygc[PH ? REPS : 1][NA];      // PH 1: the probabilities of the frames whose gradient THIS wave forms
        int rb_cur = block_rows(t_begin);
#pragma unroll
        for (int i = 0; i < PFr; ++i) {
            load_row((int64_t)__builtin_amdgcn_readlane(rb_cur, i) + u.row0, ycur[i]);
            if constexpr (PH) load_other(t_begin + i, ocur[i]);
        }
        if constexpr (PH) {
#pragma unroll
            for (int rep = 0; rep < REPS; ++rep)
                load_row((int64_t)__builtin_amdgcn_readlane(rb_cur, (wave + rep * W) & (PFr - 1)) + u.row0, ygc[rep]);
        }
        int rb_nxt = block_rows(t_begin + PFr);
        for (int tb = t_begin; tb < t_end && !skip; tb += PFr) {
            RI ynxt[PFr][NA];
            BlkU onxt[PH ? PFr : 1];
            RI ygn[PH ? REPS : 1][NA];
#pragma unroll
            for (int i = 0; i < PFr; ++i) {
                load_row((int64_t)__builtin_amdgcn_readlane(rb_nxt, i) + u.row0, ynxt[i]);
                if constexpr (PH) load_other(tb + PFr + i, onxt[i]);
            }
            if constexpr (PH) {
#pragma unroll
                for (int rep = 0; rep < REPS; ++rep)
                    load_row((int64_t)__builtin_amdgcn_readlane(rb_nxt, (wave + rep * W) & (PFr - 1)) + u.row0, ygn[rep]);
            }
            const int rb_next2 = block_rows(tb + 2 * PFr);
            // the block's probabilities per state, gathered before the serial part starts (kept in their storage type: a
            // float64 copy of a block's 8 x 3 values is 24 more registers, and eight waves leave 256 each)
            RI ybv[PFr], ylv[PFr][KH];
#pragma unroll
            for (int i = 0; i < PFr; ++i) {
                ybv[i] = (RI)bcast(ycur[i], blank);
#pragma unroll
                for (int jj = 0; jj < KH; ++jj) {
                    const RI g = (RI)gather(ycur[i], lab[jj]);
                    ylv[i][jj] = valid_lab[jj] ? g : (RI)0;
                }
            }
            auto post = [&](int i) {
                if constexpr (PH) {
                    products(i, ocur[i]);
                } else {
                    store_row(tb + i);
                }
            };
            const bool fast = (tb + PFr - 1 < t_end) && (L <= 2 * (T - (tb + PFr - 1)));
            if (fast) {
#pragma unroll
                for (int i = 0; i < PFr; ++i) {
                    R yl[KH];
#pragma unroll
                    for (int jj = 0; jj < KH; ++jj) yl[jj] = (R)ylv[i][jj];
                    step(std::true_type(), tb + i, (R)ybv[i], yl);
                    post(i);
                }
            } else {
#pragma unroll
                for (int i = 0; i < PFr; ++i) {
                    if (tb + i < t_end) {
                        R yl[KH];
#pragma unroll
                        for (int jj = 0; jj < KH; ++jj) yl[jj] = (R)ylv[i][jj];
                        step(std::false_type(), tb + i, (R)ybv[i], yl);
                        post(i);
                    }
                }
            }
            if constexpr (PH) grad_block(tb, t_end, rb_cur, ygc);
            if (first_bad != NO_BAD) skip = 1;
#pragma unroll
            for (int i = 0; i < PFr; ++i) {
#pragma unroll
                for (int q = 0; q < NA; ++q) ycur[i][q] = ynxt[i][q];
                if constexpr (PH) ocur[i] = onxt[i];
            }
            if constexpr (PH) {
#pragma unroll
                for (int rep = 0; rep < REPS; ++rep)
#pragma unroll
                    for (int q = 0; q < NA; ++q) ygc[rep][q] = ygn[rep][q];
            }
            rb_cur = rb_nxt;
            rb_nxt = rb_next2;
        }
    };

    // meet the partner workgroup: publish `mine_val` (> 0) in my word, wait (bounded, ~0.5 s) for the partner's;
    // 0 = the partner never showed up.  Release before (every wave: its stores are written back), acquire behind.
    auto meet = [&](int word, int mine_val) -> int {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_store(&sync[word + dir], (uint32_t)mine_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t v = 0;
            for (int spins = 0; spins < (1 << 22); ++spins) {
                v = __hip_atomic_load(&sync[word + (dir ^ 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v != 0) break;
                __builtin_amdgcn_s_sleep(8);
            }
            sh_word = (int32_t)v;
        }
        __syncthreads();
        const int got = sh_word;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __syncthreads();          // sh_word may be written again
        return got;
    };

    // ---- tau = 0 (ctc_fast.pyx:42-47 / :79-84); it belongs to phase 1 only when T == 1 (alpha stores nothing)
    RI y0[NA];
    int row_first;
    {
        const int t = dir ? T - 1 : 0;
        row_first = p.rowbase ? p.rowbase[t] : t;
        load_row((int64_t)row_first + u.row0, y0);
        const R yb = bcast(y0, blank);
        const R yl = gather(y0, lab[0]);
        if (gl == 0) { a[0] = yb; a[1] = yl; }
        const R c = block_sum(a[0] + a[1], a[K - 1], 0);
        if (c == (R)0) {
            skip = 1;   // ZeroDivisionError at :45
            first_bad = 0;
        } else {
            const R r = recip(c);
            a[0] *= r;
            a[1] *= r;
            rprev = r;
            ll_account(c);
        }
        if (dir == 0 && gl < K) mine[gl - K] = (ST)0;      // the pad in front of my first row (beta reads across it)
        if (Tst > 0) store_row(0);
        run(std::integral_constant<int, 0>(), 1, Tst);
    }
    int timed_out = 0;
    {
        const int got = meet(0, 1 + skip);
        timed_out |= got == 0;
        // the partner failed in phase 0 (or never came): nothing to multiply with.  Alpha goes on all the same when beta has
        // failed: the zero band sum lies behind the middle, and the cost is -llForward as far as ALPHA gets
        // (ctc_fast.pyx:147-149) -- it meets the same zero in its phase 1; what it multiplies and writes on the way is
        // taken back below like every row of an utterance that skips
        if (got == 0 || (got != 1 && dir == 1)) skip |= 2;
    }
    load_lists();
    if (Tst == 0 && !skip) {
        // T == 1, alpha: the one frame's gradient against beta's stored row 0
        BlkU ob;
        load_other(0, ob);
        products(0, ob);
        lds_barrier();
        if (wave == 0) grad_frame(std::integral_constant<int, 0>(), 0, (int64_t)row_first + u.row0, true, y0);
    }
    // (p.diag, SCTC_CTC_DIAG -- timing experiments, results are wrong: 1 = no phase 1)
    run(std::integral_constant<int, 1>(), Tst > 0 ? Tst : 1, (p.diag & 1) ? 0 : T);

    // ---- the verdicts of both directions; cost and skip flag (alpha's workgroup)
    const int mine_skip = (skip & 1) | (first_bad != NO_BAD ? 1 : 0);
    const int got = meet(2, 1 + mine_skip);
    timed_out |= got == 0;
    const int any_skip = mine_skip | (got == 2 ? 1 : 0);
    if (dir == 0 && threadIdx.x == 0) {
        double cost = llf.neg_log();   // -llForward (ctc_fast.pyx:149,152)
        if (empty_band && !mine_skip) cost = INFINITY;   // math.log(0.0)
        if (timed_out) cost = NAN;
        p.cost[b] = cost;
        p.skip[b] = any_skip;
    }
    if (any_skip || timed_out) {
        // the reference returns its zero-initialised grad (ctc_fast.pyx:31-32,149): the rows this direction is
        // responsible for are taken back (alpha: t >= Ta, beta: t < Ta)
        const int t0 = dir ? 0 : Ta, t1 = dir ? Ta : T;
        for (int t = t0 + wave; t < t1; t += W) {
            RI* gr = grad + ((int64_t)(p.rowbase ? p.rowbase[t] : t) + u.row0) * ld;
            for (int k = lane; k < A; k += 64) gr[k] = (RI)0;
        }
    }
}

// ---------------------------------------------------------------- launcher: the plan's (store, K, W, NA) -> one instantiation

template <typename RI, typename ST, int K, int NA, int W>
static int launch_fusedw_one(const CtcFusedArgs<RI>& a, int B, hipStream_t stream)
{
    constexpr int NT = 64 * W, KH = K / 2;
    constexpr int PF = NA * (int)sizeof(RI) >= 16 ? 4 : 8;
    const size_t dyn = sizeof(double) * PF * NT * K + sizeof(int32_t) * (NT * KH + a.A + 1);
    static std::once_flag once;     // one per instantiation
    static hipError_t attr = hipSuccess;
    std::call_once(once, [&] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&ctc_fusedw_kernel<RI, ST, K, NA, W>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
    });
    SCTC_HIP_TRY(attr);
    SCTC_HIP_TRY(hipMemsetAsync(a.sync, 0, sizeof(uint32_t) * FUSEDW_SYNC_WORDS * (size_t)B, stream));
    dim3 grid((unsigned)((B + 7) / 8 * 16)), block(NT);
    hipLaunchKernelGGL((ctc_fusedw_kernel<RI, ST, K, NA, W>), grid, block, dyn, stream, a, B);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

template <typename RI, typename ST, int K, int W>
static int launch_fusedw_k(const CtcFusedArgs<RI>& a, const CtcPlan& plan, hipStream_t stream)
{
    if (plan.NA == 1) return launch_fusedw_one<RI, ST, K, 1, W>(a, plan.B, stream);
    if (plan.NA == 2) return launch_fusedw_one<RI, ST, K, 2, W>(a, plan.B, stream);
    if (plan.NA == 4) return launch_fusedw_one<RI, ST, K, 4, W>(a, plan.B, stream);
    return set_error(SCTC_ERR_ARG, "ctc: no wide fused kernel for NA=%d", plan.NA);
}

template <typename RI, typename ST>
static int launch_fusedw_st(const CtcFusedArgs<RI>& a, const CtcPlan& plan, hipStream_t stream)
{
    const int K = plan.K, W = plan.W;
    if (W == 4 && K == 2) return launch_fusedw_k<RI, ST, 2, 4>(a, plan, stream);
    if (W == 4 && K == 4) return launch_fusedw_k<RI, ST, 4, 4>(a, plan, stream);
    if (W == 8 && K == 2) return launch_fusedw_k<RI, ST, 2, 8>(a, plan, stream);
    if (W == 8 && K == 4) return launch_fusedw_k<RI, ST, 4, 8>(a, plan, stream);
    return set_error(SCTC_ERR_ARG, "ctc: no wide fused kernel for K=%d, W=%d", K, W);
}

template <typename RI>
int launch_ctc_fusedw(const CtcFusedArgs<RI>& a, const CtcPlan& plan, hipStream_t stream)
{
    if constexpr (sizeof(RI) == 4) {
        if (plan.store_bytes == 4) return launch_fusedw_st<RI, uint32_t>(a, plan, stream);
    }
    if (plan.store_bytes == 8) return launch_fusedw_st<RI, double>(a, plan, stream);
    return set_error(SCTC_ERR_ARG, "ctc: no wide fused kernel for %d-byte rows", plan.store_bytes);
}

template int launch_ctc_fusedw<float>(const CtcFusedArgs<float>&, const CtcPlan&, hipStream_t);
template int launch_ctc_fusedw<double>(const CtcFusedArgs<double>&, const CtcPlan&, hipStream_t);

}  // namespace sctc
