// The kernels of the BRNN engine's MWER step (brnn_mwer.hip), as brnn_engine.hip launches them.
#pragma once
#include "common.h"

namespace sctc {

// Packed layout: frame t of rank r is row rowbase[t] + r of probs / dlogits ([N][ld]) for r < nact[t], i.e. t < Ts[r];
// slot s of that row is row (rowbase[t] + r) * S + s of kprobs / kgrad ([N * S][A]).  rowbase_S[t] = rowbase[t] * S.
struct BrnnMwerArgs {
    const float* probs;         // spread
    float* dlogits;             // combine
    int64_t ld;
    float* kprobs;
    float* kgrad;
    const int32_t* rowbase;     // [Tmax]
    const int32_t* rowbase_S;   // [Tmax]
    const int32_t* Ts;          // [B] rank order
    const int32_t* kb;          // [B] rank order, 0..K
    const int32_t* src;         // [B * S] BRNN_MWER_SRC_* or the slot's row in the CTC batch
    const double* ctc_cost;     // [rows of the CTC batch]
    const int32_t* ctc_skip;
    double* cost;               // [B * K]
    int32_t* skip;
    double* ref_cost;           // [B]
    int32_t* ref_skip;
    const double* coef;         // [B * K]
    const int32_t* real;        // [B * K]
    const int32_t* inactive;    // [B]
    double ctc_weight;
    int32_t B, K, S, A, Tmax;
};

// caller order <- rank order; loss_out[b] = loss + ctc_weight * ref_cost where the reference row is usable
struct BrnnMwerResults {
    const int32_t* perm;        // [B] rank -> caller index
    const double *loss, *expected, *post, *ref_cost;
    const int32_t *inactive, *real, *ref_skip;
    double *out_loss, *out_expected, *out_post, *out_ctc_cost;
    int32_t *out_inactive, *out_real, *out_ctc_skip;
    double ctc_weight;
    int32_t B, K, with_ref;
};

int launch_brnn_mwer_spread(const BrnnMwerArgs& a, hipStream_t s);
int launch_brnn_mwer_empty(const BrnnMwerArgs& a, hipStream_t s);
int launch_brnn_mwer_combine(const BrnnMwerArgs& a, hipStream_t s);
int launch_brnn_mwer_results(const BrnnMwerResults& a, hipStream_t s);

}  // namespace sctc
