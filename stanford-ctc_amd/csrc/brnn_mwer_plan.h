// How the MWER step of the BRNN engine (sctc_brnn_mwer_cost_and_grad, brnn_mwer.hip) lays out its
// workspace: a pure function of plain integers (host only, no HIP header: tests/test_brnn_mwer_plan_cpu.py compiles this
// file with g++).  brnn_engine.hip validates, plans, uploads and launches; the kernels decide nothing.
//
// The packed minibatch has N frames (rows) over B utterances in rank order (longest first).  Every row has S slots: the
// K hypothesis ranks and, with a reference term (ctc_weight > 0), one more for the reference label row.  Slot s of row
// `row` is row  row * S + s  of the two K-fold buffers, whose row stride is A floats, unpadded: the S * A floats of one
// frame are contiguous, as in ctc_mwer.hip, and the CTC kernels take any stride >= A.
// Workspace, every slice rounded up to 256 bytes, in this order:
//   errors    B * K double, rank order                                        | uploaded (one span: the head)
//   rowbase   Tmax int32: rowbase[t] * S                                      | uploaded
//   kb        B int32: K_b, rank order                                        | uploaded
//   src       B * S int32: the slot's row in the CTC batch, -1 an empty       | uploaded
//             hypothesis, -2 a slot that is not read
//   kprobs    N * S * A float: the probabilities of every slot a row owns
//   kgrad     N * S * A float: the CTC gradient rows of those slots
//   ctc_cost  B * S double, ctc_skip B * S int32: what the CTC call returns, in the order of its batch
//   cost      B * K double, skip B * K int32: the same per (rank, k), with the empty hypotheses and the slots not read
//   ref_cost  B double, ref_skip B int32: the reference rows, rank order
//   coef, post B * K double; real B * K int32; loss, expected B double; inactive B int32: ctc_mwer_coef_kernel's outputs
//   out_*     the seven outputs in caller order: loss, expected, ctc_cost B double; posterior B * K double; inactive,
//             ctc_skip B int32; real B * K int32
//   ctc       the CTC workspace of the batch of label rows (ctc_plan.h sizes it)
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sctc {

constexpr int BRNN_MWER_MAX_K = 256;    // MWER_MAX_K of ctc_mwer.hip
constexpr int BRNN_MWER_SRC_EMPTY = -1, BRNN_MWER_SRC_UNREAD = -2;

static inline size_t brnn_mwer_align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct BrnnMwerPlan {
    int32_t B = 0, K = 0, S = 0, A = 0, Tmax = 0;
    int64_t N = 0;
    int64_t ldk = 0;        // row stride of the K-fold buffers in floats
    size_t off_errors = 0, off_rowbase = 0, off_kb = 0, off_src = 0, head_bytes = 0;
    size_t off_kprobs = 0, off_kgrad = 0;
    size_t off_ctc_cost = 0, off_ctc_skip = 0, off_cost = 0, off_skip = 0, off_ref_cost = 0, off_ref_skip = 0;
    size_t off_coef = 0, off_post = 0, off_real = 0, off_loss = 0, off_expected = 0, off_inactive = 0;
    size_t off_out_loss = 0, off_out_expected = 0, off_out_ctc_cost = 0, off_out_post = 0, off_out_inactive = 0,
           off_out_ctc_skip = 0, off_out_real = 0;
    size_t off_ctc = 0, ctc_bytes = 0;
    size_t bytes = 0;
};

// N * S <= INT32_MAX, 1 <= K <= BRNN_MWER_MAX_K validated by the caller
static inline BrnnMwerPlan brnn_mwer_plan(int32_t B, int32_t K, bool with_ref, int32_t A, int64_t N, int32_t Tmax,
                                          size_t ctc_bytes)
{
    BrnnMwerPlan p;
    p.B = B;
    p.K = K;
    p.S = K + (with_ref ? 1 : 0);
    p.A = A;
    p.N = N;
    p.Tmax = Tmax;
    p.ldk = A;
    const size_t BK = (size_t)B * K, BS = (size_t)B * p.S, D = sizeof(double), I = sizeof(int32_t);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += brnn_mwer_align256(bytes); return o; };
    p.off_errors = take(BK * D);
    p.off_rowbase = take((size_t)Tmax * I);
    p.off_kb = take((size_t)B * I);
    p.off_src = take(BS * I);
    p.head_bytes = at;
    const size_t kfold = (size_t)N * p.S * (size_t)p.ldk * sizeof(float);
    p.off_kprobs = take(kfold);
    p.off_kgrad = take(kfold);
    p.off_ctc_cost = take(BS * D);
    p.off_ctc_skip = take(BS * I);
    p.off_cost = take(BK * D);
    p.off_skip = take(BK * I);
    p.off_ref_cost = take((size_t)B * D);
    p.off_ref_skip = take((size_t)B * I);
    p.off_coef = take(BK * D);
    p.off_post = take(BK * D);
    p.off_real = take(BK * I);
    p.off_loss = take((size_t)B * D);
    p.off_expected = take((size_t)B * D);
    p.off_inactive = take((size_t)B * I);
    p.off_out_loss = take((size_t)B * D);
    p.off_out_expected = take((size_t)B * D);
    p.off_out_ctc_cost = take((size_t)B * D);
    p.off_out_post = take(BK * D);
    p.off_out_inactive = take((size_t)B * I);
    p.off_out_ctc_skip = take((size_t)B * I);
    p.off_out_real = take(BK * I);
    p.off_ctc = at;
    p.ctc_bytes = ctc_bytes;
    at += brnn_mwer_align256(ctc_bytes);
    p.bytes = at;
    return p;
}

}  // namespace sctc
