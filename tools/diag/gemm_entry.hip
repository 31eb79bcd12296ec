// Test-only door to sctc::launch_gemm_f32(GemmArgs) and sctc::gemm_plan_splits of libsctc_hip.so: the public
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

extern "C" int sctc_diag_gemm(const sctc_diag_gemm_args* s, void* stream)
{
    if (!s) {
        snprintf(sctc::err_buf(), 512, "diag gemm: null argument struct");
        return -1;
    }
    sctc::GemmArgs g;
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
    return sctc::launch_gemm_f32(g, (hipStream_t)stream);
}

extern "C" int64_t sctc_diag_gemm_plan_splits(int32_t M, int32_t N, int32_t K, int32_t prec, int32_t in16, int32_t* splits)
{
    int s = 1;
    const int64_t need = sctc::gemm_plan_splits(M, N, K, &s, prec, in16);
    if (splits) *splits = s;
    return need;
}
