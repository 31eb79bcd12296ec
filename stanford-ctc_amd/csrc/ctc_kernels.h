// Host-visible declarations of the CTC kernels (ctc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_plan.h"

namespace sctc {

// RI = type of probs/grad in HBM (float or double).  The lattices and all lattice
// arithmetic are float64 like the reference (ctc_fast.pyx:8,28-30): a float32 lattice
// loses utterances with T >> 2U, where the states that survive the end-of-utterance band
// carry < 1e-38 of a frame's mass (measured: 0.5-6 % cost error).
template <typename RI>
struct CtcLatticeArgs {
    const CtcUtt* utts;
    const RI* probs;
    int64_t ld;
    int32_t A, blank, lp;
    const int32_t* rowbase;  // nullable
    const int32_t* labels;
    double* alpha;
    double* beta;
    double* ll;      // [2B] llForward / llBackward
    int32_t* skip2;  // [2B]
    double* scratch; // ctc_generic.hip only: [B][2 directions][2][lp] unnormalised rows
};

template <typename RI>
struct CtcGradArgs {
    const CtcUtt* utts;
    const RI* probs;
    RI* grad;
    int64_t ld;
    int32_t A, blank, lp;
    const int32_t* rowbase;
    const int32_t* labels;
    // the odd (label) states of every utterance grouped by label, ascending inside a group: by_label[lab_off + j]
    // = state index 2i+1, group k = [label_start[b*(A+1) + k], label_start[b*(A+1) + k + 1]) (host-built, capi_ctc.hip)
    const int32_t* by_label;
    const int32_t* label_start;
    const double* alpha;
    const double* beta;
    const double* ll;
    const int32_t* skip2;
    double* cost;   // [B]
    int32_t* skip;  // [B]
    int32_t lazy;   // lattices were produced with the every-4th-frame rescaling
};

// ctc_fused.hip: both recursions and the gradient in one kernel (label rows of up to 512 states).
// `store` holds, per utterance, T rows of round_up(2U+1, K) states (alpha's first T/2 frames, then
// beta's first T - T/2) behind a K-element pad, as float64 or in the 32-bit format of ctc_fused.hip;
// CtcUtt::lat_off counts elements of that type.
template <typename RI>
struct CtcFusedArgs {
    const CtcUtt* utts;
    const RI* probs;
    RI* grad;
    int64_t ld;
    int32_t A, blank;
    const int32_t* rowbase;  // nullable
    const int32_t* labels;
    const int32_t* by_label;     // as in CtcGradArgs
    const int32_t* label_start;
    void* store;
    double* cost;    // [B]
    int32_t* skip;   // [B]
    int32_t diag;    // SCTC_CTC_DIAG, timing experiments only (results are wrong): 1 no phase 1, 2 helper without
                     // finish, 4 helper without products, 8 recursion waves do not wait for the helper
    uint32_t* sync;  // ctc_fusedw.hip only: ctc_fusedw_sync_bytes(B) of flag words (the launcher zeroes them)
};
// The launchers take a plan (ctc_plan.h) and turn it into the one template instantiation it names; a combination that is
// not compiled is SCTC_ERR_ARG.
template <typename RI>
int launch_ctc_fused(const CtcFusedArgs<RI>& a, const CtcPlan& plan, hipStream_t stream);
// ctc_fusedw.hip: the same schedule for rows of 513..2048 states -- one workgroup of W = 4 / 8 waves per (utterance,
// direction), K = 2 / 4 states per lane; the store is laid out like the narrow kernel's
template <typename RI>
int launch_ctc_fusedw(const CtcFusedArgs<RI>& a, const CtcPlan& plan, hipStream_t stream);
// ctc_kernels.hip
template <typename RI>
int launch_ctc_lattice(const CtcLatticeArgs<RI>& a, const CtcPlan& plan, hipStream_t stream);
template <typename RI>
int launch_ctc_grad(const CtcGradArgs<RI>& a, const CtcPlan& plan, hipStream_t stream);
int launch_softmax_rows(const float* x, float* y, int64_t rows, int A, int64_t ld,
                        hipStream_t stream);
// ctc_generic.hip: any label length, any alphabet (rows of more than 2048 states, more than 256 symbols)
int launch_softmax_rows_generic(const float* x, float* y, int64_t rows, int A, int64_t ld, hipStream_t stream);
template <typename RI>
int launch_ctc_generic(const CtcLatticeArgs<RI>& la, const CtcGradArgs<RI>& ga, const CtcPlan& plan, hipStream_t stream);
int launch_argmax_rows(const void* y, int dtype, int32_t* best, int64_t rows, int A, int64_t ld,
                       hipStream_t stream);

// capi_ctc.hip: the workspace one sctc_ctc_loss_batch call on these utterances needs (argument checks, plan, ctc_layout)
int ctc_workspace_bytes(int B, int A, int blank, int dtype, const int32_t* T_b, const int32_t* U_b, size_t* bytes);

}  // namespace sctc
