// Device code the CTC kernels share (ctc_kernels.hip, ctc_fused.hip, ctc_fusedw.hip, ctc_generic.hip): the pieces of
// the scaled recursion of ctc_fast/ctc-loss/ctc_fast.pyx:42-114 that have to match the reference bit for bit, once.
// Device only: ctc_kernels.h and ctc_plan.h (host code, compiled by g++ in the tests) do not include it.  The structs
// hold named members only, so they dissolve into registers.
//
// What is NOT here although the kernels restate it (the per-lane label constants, the zero-band-sum latch, the geometry
// of the meet-in-the-middle row store, the tau = 0 frame): moving any of them behind a function or into a struct made
// the compiler lay out the frame loop differently (profiles/ctc_dev_refactor.md has the numbers), and this header
// holds only what leaves every kernel's registers, scratch, LDS and occupancy as they were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_plan.h"
#include "xlane.h"

namespace sctc {

using CtcR = double;   // the recursion, the normalisers and llForward are float64 like the reference (ctc_fast.pyx:8,28-30)

// ---------------------------------------------------------------- reciprocals

// 1/c for the row scaling: hardware estimate + two Newton-Raphson steps (the reciprocal part of the IEEE division
// sequence without its scaling / fix-up tail, half its dependent operations; <= 1 ulp).  Which double is applied does
// not matter for parity: the per-frame factors cancel in the gradient (ctc_fast.pyx:138-145), and llForward takes the
// logarithm of the band sums themselves (LogProduct; the lattice kernels store them beside the rows).
__device__ __forceinline__ CtcR ctc_recip(CtcR c)
{
    CtcR x = __builtin_amdgcn_rcp(c);
    CtcR e = fma(-c, x, (CtcR)1);
    x = fma(x, e, x);
    e = fma(-c, x, (CtcR)1);
    return fma(x, e, x);
}

// 1/y for absum's per-state division (:125-131); y == 0 only ever meets a product that is exactly zero (the
// reference's `ab != 0` guard).  float32 probabilities are normal float64 numbers: the Newton reciprocal; float64
// probabilities may be denormal: the IEEE division.
template <typename RI>
__device__ __forceinline__ CtcR ctc_recip_or_zero(CtcR y)
{
    if constexpr (sizeof(RI) == 4) {
        const CtcR r = ctc_recip(y);
        return y > (CtcR)0 ? r : (CtcR)0;
    } else {
        return y > (CtcR)0 ? (CtcR)1 / y : (CtcR)0;
    }
}

// ---------------------------------------------------------------- a frame's probabilities: lane k (+64q) <- y[t][k]

// value of symbol k (per lane) from the NA registers of a row; every lane takes part (cross-lane operation)
template <typename T, int NA>
__device__ __forceinline__ T row_gather(const T (&y)[NA], int k)
{
    T out = lane_gather(y[0], k & 63);
#pragma unroll
    for (int q = 1; q < NA; ++q) {
        T o = lane_gather(y[q], k & 63);
        if ((k >> 6) == q) out = o;
    }
    return out;
}

// the same for a wave-uniform k
template <typename T, int NA>
__device__ __forceinline__ T row_bcast(const T (&y)[NA], int k)
{
    T out = lane_bcast(y[0], k & 63);
#pragma unroll
    for (int q = 1; q < NA; ++q) {
        T o = lane_bcast(y[q], k & 63);
        if ((k >> 6) == q) out = o;
    }
    return out;
}

__device__ __forceinline__ int64_t frame_row(const CtcUtt& u, const int32_t* rowbase, int t)
{
    return rowbase ? (int64_t)rowbase[t] + u.row0 : u.row0 + t;
}

// The fused kernels: NO load or store of the frame loops sits under a branch, not even a lane mask.  Behind control flow
// the compiler no longer knows how many memory operations are in flight and turns every later wait into s_waitcnt
// vmcnt(0) -- a block's prefetch then waited for the rows (phase 0) or gradient rows (phase 1) stored a moment before,
// an HBM write round trip per block of frames (1.3 us per block of 8: the first version of ctc_fusedw.hip's phase 1).
// Columns are clamped and masked by a select, rows beyond the end are clamped, lanes / frames that have nothing to
// store write to a dump area nobody reads unmasked.
template <typename RI, int NA>
__device__ __forceinline__ void load_row_clamped(const RI* probs, int64_t ld, int A, int lane, int64_t row, RI (&dst)[NA])
{
    const RI* yr = probs + row * ld;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        const int k = lane + 64 * q;
        const RI v = yr[min(k, A - 1)];
        dst[q] = k < A ? v : (RI)0;
    }
}
// The lattice kernel predicates the load instead (its only stores are the lattice rows, waited for once per block anyway).
template <typename RI, int NA>
__device__ __forceinline__ void load_row_predicated(const RI* probs, int64_t ld, int A, int lane, int64_t row, RI (&dst)[NA])
{
    const RI* yr = probs + row * ld;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        const int k = lane + 64 * q;
        dst[q] = k < A ? yr[k] : (RI)0;
    }
}

// Row indices of a whole block of frames with ONE vector load (lane i <- frame tau0 + i, clamped), fetched a block
// before they are needed.  Looking rowbase[t] up frame by frame put a dependent load and an s_waitcnt vmcnt(0) -- which
// also waits for every row store in flight -- in front of each prefetched frame: 1000 of the 1600 shader cycles a frame
// cost (s_memtime stamps).
__device__ __forceinline__ int block_rows(const int32_t* rowbase, int T, int dir, int lane, int tau0)
{
    const int tau = min(tau0 + lane, T - 1);
    const int t = dir ? T - 1 - tau : tau;
    return rowbase ? rowbase[t] : t;
}
// (ctc_fused.hip keeps a variant of its own that loads unconditionally, through a table that is never null)

// ---------------------------------------------------------------- sums and barriers

// sum of a lane's K values as a balanced tree in a fixed order (log2 K dependent additions instead of K-1)
template <int K>
__device__ __forceinline__ CtcR sum_tree(const CtcR (&n)[K])
{
    CtcR t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = n[j];
#pragma unroll
    for (int w = 1; w < K; w *= 2)
#pragma unroll
        for (int j = 0; j + w < K; j += 2 * w) t[j] += t[j + w];
    return t[0];
}

// workgroup barrier that orders LDS traffic only: __syncthreads() would also drain the row / gradient stores to HBM
// (vmcnt) in every frame
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// W waves share one (utterance, direction): state s lives in global lane gl = s / K.  The two cross-wave couplings of a
// frame -- the band sum and the neighbour state of a wave's lane 0 (last state of the previous wave) -- go through the
// caller's __shared__ Slots behind ONE workgroup barrier per frame.  Before it every wave publishes its band-sum partial
// and its last state's UNNORMALISED value n[K-1] (one 16-byte slot, written by lane 63 with one ds_write_b128); after it
// every wave knows the frame's c (and r = 1/c), and the next frame's neighbour state of lane 0 is bprev * r -- the very
// multiplication the owning wave performs, so the lattice is bit-identical to the two-barrier schedule this replaces
// (publish the normalised boundary after the sum, meet again at the start of the next frame: 1.08 us per frame at
// T = 8000 / U = 800).  Slots alternate by frame parity: a wave that races ahead writes the other slot, and cannot
// reach this one again before everybody has passed the next barrier.
template <int W>
struct CrossWave {
    using Slots = double[2][W > 1 ? W : 1][2];   // per frame parity and wave: {band-sum partial, last state, unnormalised}
    CtcR bprev = (CtcR)0;   // the previous wave's last state as of the last exchange (read right behind its barrier)

    // sum over all states of the block, identical in every lane (fixed order)
    __device__ __forceinline__ CtcR sum(Slots& xw, CtcR loc, CtcR last_unnorm, int tau, int lane, int wave)
    {
        const CtcR ws = wave_sum(loc);
        if constexpr (W == 1) {
            return ws;
        } else {
            if (lane == 63) *reinterpret_cast<double2*>(&xw[tau & 1][wave][0]) = make_double2(ws, last_unnorm);
            lds_barrier();
            // every read behind the barrier is issued at once: the W partials and the boundary state the NEXT frame
            // needs (it used to be a dependent LDS read at the head of that frame)
            CtcR pw[W];
#pragma unroll
            for (int w = 0; w < W; ++w) pw[w] = xw[tau & 1][w][0];
            bprev = xw[tau & 1][wave > 0 ? wave - 1 : 0][1];
            return sum_tree(pw);
        }
    }
    // frames without a rescale (the lattice kernel's lazy schedule): the boundary state alone
    __device__ __forceinline__ void publish(Slots& xw, CtcR last, int tau, int lane, int wave)
    {
        if constexpr (W > 1) {
            if (lane == 63) xw[tau & 1][wave][1] = last;
            lds_barrier();
            bprev = xw[tau & 1][wave > 0 ? wave - 1 : 0][1];
        }
    }
    // last state of global lane gl - 1 as of the previous frame (start of a frame); rprev = the factor the previous
    // frame's row was scaled with (1 if it was not)
    __device__ __forceinline__ CtcR shift_in(CtcR last, CtcR rprev, int lane, int wave) const
    {
        CtcR prev = lane_shr1(last);
        if constexpr (W > 1) {
            const CtcR across = bprev * rprev;          // the very product the owning wave formed
            prev = (lane == 0 && wave > 0) ? across : prev;
        }
        return prev;
    }
};

// ---------------------------------------------------------------- the recursion

// One frame of the recursion (ctc_fast.pyx:58-68) is NOT here: each of the three kernels states it in its `step` /
// frame loop.  As a shared function it changed bits -- the compiler contracts the band sum n[0] + n[1] of two products
// into an fma with one of them, and behind a function boundary it picked the other one (float64 probabilities, all
// fused kernels) -- and in the lattice kernel it changed the register allocation of 62 kernels.  So the bits pinned in
// tests/data/ctc_bits_parent.txt hang on which product the compiler's default -ffp-contract fuses there: a compiler
// upgrade may move them with no source change (then record again); writing that fma out by hand would end the
// dependence, and change the bits once -- not done here.  What the copies share:
// FAST frames, whose band starts at state 0 (L <= 2(T - tau): all but the last ~U frames), need no band test, and the
// states beyond the label row stay exactly zero because their label probability was zeroed at gather time (a blank
// state beyond the row only ever adds zeros).  The step is then 2 DPP moves and 5 float64 operations per state pair --
// no compares or selects on the recursion's dependency chain.  `in + allow*below` as one fma rounds like the add.

// llForward = sum_t log c_t (ctc_fast.pyx:47,76) = log of the product of the band sums c_t: the product is carried as
// mantissa x 2^exponent (three operations per frame, beside the recursion's chain) and its logarithm taken once; the
// caller passes 1 for frames from the first zero band sum on (the reference's exception leaves llForward as it was,
// :147-149).  The product of the c_t themselves, not of the applied factors 1/c_t: for T = 1 the cost is then the
// logarithm of the very double the reference takes it of (a cost of 1e-8 -- one frame, c = 1 - 1e-8 -- would otherwise
// carry the reciprocal's rounding: 2e-8 relative, found by the fuzz test).
struct LogProduct {
    CtcR m = (CtcR)1;
    int e = 0;
    __device__ __forceinline__ void account(CtcR f)
    {
        m *= f;
        e += __builtin_amdgcn_frexp_exp(m);
        m = __builtin_amdgcn_frexp_mant(m);
    }
    // -llForward (ctc_fast.pyx:149,152).  Mantissa in [sqrt(1/2), sqrt(2)): a product near 1 has exponent 0 and its
    // logarithm no cancellation against exponent x ln 2
    __device__ __forceinline__ double neg_log()
    {
        if (m < 0.70710678118654752440) {
            m *= 2.0;
            e -= 1;
        }
        return -(log(m) + (double)e * 0.693147180559945309417232121458);
    }
};

}  // namespace sctc
