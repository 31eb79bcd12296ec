// Prints decisions of csrc/bwd_overlap_plan.h, csrc/recurrent_plan.h and csrc/gemm_plan.h for the overlap order of the
// backward pass (tests/test_bwd_overlap_plan_cpu.py compiles this with g++).
//   bwd_overlap_plan_dump rec      "rec Hp B prec16 variant: name grid lds" of the first candidate, variants 0, 52, 53
//   bwd_overlap_plan_dump lds      "gemm shape lds_bytes" of every fp32 tile shape, "claim bytes", "cu bytes"
//   bwd_overlap_plan_dump elig     "elig NL TL Hp fp32 train B: config eligible extra"
//   bwd_overlap_plan_dump route    "route NL TL overlap: ok check | d_in/d_out/deferred per loop index NL .. 0"
#include <stdio.h>
#include <string.h>

#include "bwd_overlap_plan.h"
#include "gemm_plan.h"
#include "recurrent_plan.h"

using namespace sctc;

static void rec()
{
    for (int Hp : {512, 1024, 1824, 2048})
        for (int B : {1, 16, 17, 24, 32, 33, 64})
            for (int p16 = 0; p16 < 2; ++p16)
                for (int v : {0, 52, 53}) {
                    RecCandidate c[REC_MAX_CANDIDATES];
                    const RecShape s = {Hp, B, p16, 1, v, 0, 256};
                    const int n = rec_plan(s, c);
                    if (n < 1) { printf("rec %d %d %d %d: rejected\n", Hp, B, p16, v); continue; }
                    char name[96];
                    rec_candidate_name(c[0], name, sizeof(name));
                    printf("rec %d %d %d %d: %s | %d %zu %d %d", Hp, B, p16, v, name, c[0].grid, c[0].lds, c[0].variant, c[0].ntarg);
                    for (int i = 0; i < c[0].ntarg; ++i) printf(" %d", c[0].targ[i]);
                    printf("\n");
                }
}

static void lds()
{
    for (int shape = 0; shape < GEMM_N_SHAPES; ++shape) {
        GemmSwitches sw;
        sw.shape = shape;
        GemmQuery q;
        q.M = q.N = 1824;
        q.K = 32000;
        printf("gemm %d %d\n", shape, gemm_plan(q, sw).lds_bytes);
    }
    printf("claim %zu\n", REC_LDS_EXCLUDES_GEMM);
    printf("cu %zu\n", REC_LDS_MAX);
}

static void elig()
{
    for (int NL = 1; NL <= 7; ++NL)
        for (int TL = 0; TL <= NL; ++TL)
            for (int Hp : {1024, 1824, 2048})
                for (int fp32 = 0; fp32 < 2; ++fp32)
                    for (int train = 0; train < 2; ++train)
                        for (int B : {1, 16, 17, 32, 33})
                            printf("elig %d %d %d %d %d %d: %d %d %d\n", NL, TL, Hp, fp32, train, B,
                                   (int)bwd_overlap_config_ok(NL, TL, Hp, fp32, train),
                                   (int)bwd_overlap_eligible(NL, TL, Hp, fp32, train, B),
                                   bwd_overlap_extra_bufs(NL, TL, Hp, fp32, train));
}

static void route()
{
    for (int NL = 1; NL <= 7; ++NL)
        for (int TL = 0; TL <= NL; ++TL)
            for (int ov = 0; ov < 2; ++ov) {
                BwdRoute r;
                const bool ok = bwd_route(NL, TL, ov, &r);
                printf("route %d %d %d: %d %d |", NL, TL, ov, (int)ok, ok ? bwd_route_check(NL, TL, ov, r) : -1);
                for (int i = NL; ok && i >= 0; --i) printf(" %d/%d/%d", r.d_in[i], r.d_out[i], (int)r.deferred[i]);
                printf("\n");
            }
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "rec")) rec();
    else if (argc == 2 && !strcmp(argv[1], "lds")) lds();
    else if (argc == 2 && !strcmp(argv[1], "elig")) elig();
    else if (argc == 2 && !strcmp(argv[1], "route")) route();
    else return 2;
    return 0;
}
