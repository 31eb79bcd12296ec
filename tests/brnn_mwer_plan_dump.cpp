// Prints the workspace layout of csrc/brnn_mwer_plan.h (tests/test_brnn_mwer_plan_cpu.py compiles this with g++).
//   stdin: lines "B K with_ref A N Tmax ctc_bytes"
//   per line: "plan S ldk head_bytes ctc_bytes bytes", then "slice name offset bytes align" per slice in workspace
//   order (align: what its reader assumes), then "end"
#include <stdio.h>

#include "brnn_mwer_plan.h"

using namespace sctc;

int main()
{
    int B, K, with_ref, A, Tmax;
    long long N;
    size_t ctc;
    while (scanf("%d %d %d %d %lld %d %zu", &B, &K, &with_ref, &A, &N, &Tmax, &ctc) == 7) {
        const BrnnMwerPlan p = brnn_mwer_plan(B, K, with_ref != 0, A, N, Tmax, ctc);
        const size_t BK = (size_t)B * K, BS = (size_t)B * p.S, D = sizeof(double), I = sizeof(int32_t);
        const size_t kfold = (size_t)N * p.S * (size_t)p.ldk * sizeof(float);
        printf("plan %d %lld %zu %zu %zu\n", p.S, (long long)p.ldk, p.head_bytes, p.ctc_bytes, p.bytes);
        struct { const char* name; size_t off, bytes, align; } s[] = {
            {"errors", p.off_errors, BK * D, 8}, {"rowbase", p.off_rowbase, (size_t)Tmax * I, 4}, {"kb", p.off_kb, B * I, 4},
            {"src", p.off_src, BS * I, 4}, {"kprobs", p.off_kprobs, kfold, 256}, {"kgrad", p.off_kgrad, kfold, 256},
            {"ctc_cost", p.off_ctc_cost, BS * D, 8}, {"ctc_skip", p.off_ctc_skip, BS * I, 4}, {"cost", p.off_cost, BK * D, 8},
            {"skip", p.off_skip, BK * I, 4}, {"ref_cost", p.off_ref_cost, B * D, 8}, {"ref_skip", p.off_ref_skip, B * I, 4},
            {"coef", p.off_coef, BK * D, 8}, {"post", p.off_post, BK * D, 8}, {"real", p.off_real, BK * I, 4},
            {"loss", p.off_loss, B * D, 8}, {"expected", p.off_expected, B * D, 8}, {"inactive", p.off_inactive, B * I, 4},
            {"out_loss", p.off_out_loss, B * D, 8}, {"out_expected", p.off_out_expected, B * D, 8},
            {"out_ctc_cost", p.off_out_ctc_cost, B * D, 8}, {"out_post", p.off_out_post, BK * D, 8},
            {"out_inactive", p.off_out_inactive, B * I, 4}, {"out_ctc_skip", p.off_out_ctc_skip, B * I, 4},
            {"out_real", p.off_out_real, BK * I, 4}, {"ctc", p.off_ctc, p.ctc_bytes, 256},
        };
        for (const auto& q : s) printf("slice %s %zu %zu %zu\n", q.name, q.off, q.bytes, q.align);
        printf("end\n");
    }
    return 0;
}
