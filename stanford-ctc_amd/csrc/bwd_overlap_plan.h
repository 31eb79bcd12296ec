// The backward pass's overlap of the weight gradients above the temporal layer with the BPTT recurrence: when it applies
// and which delta buffer every GEMM of the pass writes and reads.  Pure functions of plain integers (host only, no HIP
// header: tests/test_bwd_overlap_plan_cpu.py and tests/bwd_overlap_route_check.cpp compile this file with g++).
// brnn_engine.hip (run_backward) launches what this file decides.
//
// Serial order (mode 0), loop index i = NL .. 0:  dW_i = d_in_i . act_i ; d_out_i = W_i^T d_in_i ; BPTT behind i == TL.
// Overlap order: the delta GEMMs of i = NL .. TL back to back, the BPTT grid, and -- beside it, on a stream of their own
// and on the CUs it leaves free -- the weight gradients of i = NL .. TL ("deferred"), joined behind the BPTT.  A deferred
// gradient reads its d_in AFTER every delta GEMM in front of the join has run, so none of those may write a buffer a
// deferred gradient still reads: they take NL - TL + 1 different buffers (the serial order ping-pongs between two).
#pragma once

namespace sctc {

// SCTC_BWD_OVERLAP
enum BwdOverlapMode : int {
    BWD_OVERLAP_OFF = 0,    // the serial order
    BWD_OVERLAP_CLAIM = 1,  // beside the default BPTT grid (Hp / 8 CUs) launched with REC_V_T_CLAIM
    BWD_OVERLAP_HALF = 2,   // beside the half-grid BPTT (REC_V_T_HALF, Hp / 16 CUs)
};
// what an unset switch means: the measured choice (profiles/bwd_overlap.md)
static constexpr int BWD_OVERLAP_DEFAULT = BWD_OVERLAP_HALF;

// delta buffers: the CTC gradient, the serial order's ping-pong pair, the overlap order's extra ones
enum BwdBuf : int { BWD_BUF_LOGITS = 0, BWD_BUF_A = 1, BWD_BUF_B = 2, BWD_BUF_X0 = 3 };
static constexpr int BWD_MAX_EXTRA = 5;         // extra delta buffers a handle may carve
static constexpr int BWD_MAX_LAYERS = 64;       // loop indices a BwdRoute holds

// H x H weight gradients above the temporal layer: loop indices TL .. NL - 1 (NL is the output layer's)
static inline int bwd_overlap_hh_above(int NL, int TL) { return TL > 0 && TL < NL ? NL - TL : 0; }

// What the handle's configuration allows (carve: the extra buffers exist exactly then).  TL <= 0: no temporal layer.
// At least two H x H gradients above it: with one, the half grid's longer BPTT is not paid back.
static inline bool bwd_overlap_config_ok(int NL, int TL, int Hp, bool fp32, bool train)
{
    const int hh = bwd_overlap_hh_above(NL, TL);
    return train && fp32 && (Hp == 1824 || Hp == 2048) && hh >= 2 && hh - 1 <= BWD_MAX_EXTRA && NL < BWD_MAX_LAYERS;
}
static inline int bwd_overlap_extra_bufs(int NL, int TL, int Hp, bool fp32, bool train)
{
    return bwd_overlap_config_ok(NL, TL, Hp, fp32, train) ? bwd_overlap_hh_above(NL, TL) - 1 : 0;
}
// ... and a step of B utterances: the two overlap forms of the BPTT exist at 17..32 (recurrent_plan.h)
static inline bool bwd_overlap_eligible(int NL, int TL, int Hp, bool fp32, bool train, int B)
{
    return bwd_overlap_config_ok(NL, TL, Hp, fp32, train) && B >= 17 && B <= 32;
}

struct BwdRoute {
    int d_in[BWD_MAX_LAYERS];       // BwdBuf read by dW_i and by the delta GEMM of i
    int d_out[BWD_MAX_LAYERS];      // BwdBuf the delta GEMM of i writes (i >= 1; -1 for i == 0)
    bool deferred[BWD_MAX_LAYERS];  // dW_i runs beside the BPTT grid
};

// The buffers of a pass over loop indices NL .. 0.  !overlap: dA, dBuf, dA, ... as ever.  overlap (eligible only): the delta
// GEMMs in front of the join (i = NL .. TL) write A, B, X0, X1, ... in turn, the ones behind it A, B, A, ...
static inline bool bwd_route(int NL, int TL, bool overlap, BwdRoute* r)
{
    if (NL < 0 || NL >= BWD_MAX_LAYERS) return false;
    if (overlap && (bwd_overlap_hh_above(NL, TL) < 2 || bwd_overlap_hh_above(NL, TL) - 1 > BWD_MAX_EXTRA)) return false;
    int d_in = BWD_BUF_LOGITS;
    for (int i = NL; i >= 0; --i) {
        r->d_in[i] = d_in;
        r->deferred[i] = overlap && i >= TL;
        r->d_out[i] = -1;
        if (i == 0) break;
        // k-th delta GEMM of its stretch: in front of the join A, B, X0, X1, ... (the delta of layer TL itself takes the last
        // extra buffer: the BPTT's additive term, and where the next gradient's fused sum of the two BPTT outputs is
        // stored, behind the join); behind it, and in the serial order, A, B, A, ...
        const bool front = overlap && i >= TL;
        const int k = front || !overlap ? NL - i : TL - 1 - i;
        r->d_out[i] = front && k >= 2 ? BWD_BUF_X0 + (k - 2) : (k % 2 ? BWD_BUF_B : BWD_BUF_A);
        d_in = r->d_out[i];
    }
    return true;
}

// The rule the route must keep, checked on the launch order itself: every launch reads what the LAST write to its buffer
// in front of it left, and that write is its own producer's.  Serial: [dW_i, delta_i] for i = NL .. 0.  Overlap:
// delta_NL .. delta_TL, then dW_NL .. dW_TL, then [dW_i, delta_i] for i = TL - 1 .. 0.  Also: a delta GEMM never writes the
// buffer it reads.  Returns 0, or the loop index + 1 of the first launch that would read something else.
static inline int bwd_route_check(int NL, int TL, bool overlap, const BwdRoute& r)
{
    int writer[BWD_BUF_X0 + BWD_MAX_EXTRA + 1];     // loop index whose delta GEMM wrote the buffer last; NL + 1: the CTC gradient
    for (int& w : writer) w = -1;
    writer[BWD_BUF_LOGITS] = NL + 1;
    const auto read_ok = [&](int i) { return r.d_in[i] >= 0 && r.d_in[i] <= BWD_BUF_X0 + BWD_MAX_EXTRA && writer[r.d_in[i]] == i + 1; };
    const auto delta = [&](int i) {
        if (!read_ok(i) || r.d_out[i] <= BWD_BUF_LOGITS || r.d_out[i] > BWD_BUF_X0 + BWD_MAX_EXTRA || r.d_out[i] == r.d_in[i]) return false;
        writer[r.d_out[i]] = i;
        return true;
    };
    const int first_serial = overlap ? TL - 1 : NL;
    if (overlap) {
        for (int i = NL; i >= TL; --i) if (i >= 1 && !delta(i)) return i + 1;
        for (int i = NL; i >= TL; --i) if (!r.deferred[i] || !read_ok(i)) return i + 1;
    }
    for (int i = first_serial; i >= 0; --i) {
        if (r.deferred[i] || !read_ok(i)) return i + 1;
        if (i >= 1 && !delta(i)) return i + 1;
    }
    return 0;
}

}  // namespace sctc
