// Test-only door to sctc::launch_gemm_f32(GemmArgs) of libsctc_hip.so and to sctc::gemm_plan (gemm_plan.h): the public
// sctc_gemm_f32 / sctc_gemm_h16 reach only layout, bias and ReLU, the engine uses every other field of
// GemmArgs.  libsctc_diag.so LINKS against the product library, so the kernels that run are the product's.
#include <stddef.h>
#include <stdio.h>

#include "gemm_f32.h"
#include "sctc_diag.h"

namespace sctc { char* err_buf(); }     // the product library's message buffer (sctc_last_error)

// the mirror is copied field by field; a new GemmArgs field must be added to both
static_assert(sizeof(sctc_diag_gemm_args) == sizeof(sctc::GemmArgs), "sctc_diag_gemm_args: mirror out of date");
static_assert(offsetof(sctc_diag_gemm_args, a_sum) == offsetof(sctc::GemmArgs, a_sum), "sctc_diag_gemm_args: mirror out of date");

static bool mirror(const sctc_diag_gemm_args* s, sctc::GemmArgs* out)
{
    if (!s) {
        snprintf(sctc::err_buf(), 512, "diag gemm: null argument struct");
        return false;
    }
    sctc::GemmArgs& g = *out;
    g.A = (const float*)s->A; g.B = (const float*)s->B; g.C = s->C;
    g.lda = s->lda; g.ldb = s->ldb; g.ldc = s->ldc;
    g.M = s->M; g.N = s->N; g.K = s->K;
    g.a_kcontig = s->a_kcontig; g.b_kcontig = s->b_kcontig;
    g.idx_a = s->idx_a; g.idx_b = s->idx_b;
    g.bias = s->bias;
    g.mask = s->mask; g.ldmask = s->ldmask;
    g.addend = s->addend; g.ldadd = s->ldadd; g.add_scale = s->add_scale;
    g.relu = s->relu; g.accumulate = s->accumulate;
    g.colsum_a = s->colsum_a;
    g.splitk_ws = s->splitk_ws; g.splits = s->splits;
    g.prec = s->prec; g.in16 = s->in16;
    g.C16a = s->C16a; g.C16b = s->C16b; g.ldc16 = s->ldc16;
    g.skip_c32 = s->skip_c32;
    g.mask16 = s->mask16; g.ldmask16 = s->ldmask16;
    g.A2 = s->A2; g.a_sum = s->a_sum;
    return true;
}

extern "C" int sctc_diag_gemm(const sctc_diag_gemm_args* s, void* stream)
{
    sctc::GemmArgs g;
    return mirror(s, &g) ? sctc::launch_gemm_f32(g, (hipStream_t)stream) : -1;
}

extern "C" int sctc_diag_gemm_plan(const sctc_diag_gemm_args* s, sctc_diag_gemm_plan_out* out)
{
    sctc::GemmArgs g;
    if (!mirror(s, &g) || !out) return -1;
    const sctc::GemmPlan p = sctc::gemm_plan(g);
    *out = {(int32_t)p.kernel, p.bm, p.bn, p.bk, p.threads, p.occ, p.lds_bytes, p.grid_x, p.splits, p.split_tile_differs, p.ws_floats};
    return 0;
}

// The shape-only question of earlier callers, answered by the same plan: operands of one row-contiguous layout, no gather,
// leading dimensions that are multiples of 8 -- of a query the split count depends on through M, N, K, prec and in16 only.
extern "C" int64_t sctc_diag_gemm_plan_splits(int32_t M, int32_t N, int32_t K, int32_t prec, int32_t in16, int32_t* splits)
{
    const sctc::GemmPlan p = sctc::gemm_plan(sctc::GemmQuery{M, N, K, prec, in16, 0, 0}, sctc::gemm_switches_from_env());
    if (splits) *splits = p.splits;
    return p.ws_floats;
}
