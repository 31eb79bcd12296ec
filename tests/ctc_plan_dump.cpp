// Prints the decisions of csrc/ctc_plan.h (tests/test_ctc_plan_cpu.py compiles this with g++).
//   ctc_plan_dump grid     the grid of tests/data/ctc_plan_parent.txt, expanded: per case "plan L B A dtype SET" and the kernels'
//                          template-ids; per ragged batch "layout NAME dtype SET", every utterance's lat_off, the kernels
//                          (behind the first: the slice offsets) and the total bytes
//   ctc_plan_dump query    stdin: lines "B A dtype max_L max_T"; per line the kernels of that call under the switches
//                          of THIS process's environment, then "end"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ctc_plan.h"

using namespace sctc;

struct SwitchSet { const char* name; const char* env[3][2]; };
static const SwitchSet SETS[] = {
    {"default", {}},
    {"generic", {{"SCTC_CTC_GENERIC", "1"}}},
    {"lazy", {{"SCTC_CTC_LAZY", "1"}}},
    {"fused0", {{"SCTC_CTC_FUSED", "0"}}},
    {"store64", {{"SCTC_CTC_STORE", "64"}}},
    {"wide0", {{"SCTC_CTC_WIDE", "0"}}},
    {"wide1", {{"SCTC_CTC_WIDE", "1"}}},
    {"widemin1", {{"SCTC_CTC_WIDE_MIN_B", "1"}}},
    {"waves1", {{"SCTC_CTC_WAVES", "1"}}},
    {"waves4", {{"SCTC_CTC_WAVES", "4"}}},
    {"waves8", {{"SCTC_CTC_WAVES", "8"}}},
    {"helper0", {{"SCTC_CTC_HELPER", "0"}}},
    {"helper1", {{"SCTC_CTC_HELPER", "1"}}},
    {"helpermax20", {{"SCTC_CTC_HELPER_MAX_B", "20"}}},
    {"helpermax1000", {{"SCTC_CTC_HELPER_MAX_B", "1000"}}},
    {"dietmin1", {{"SCTC_CTC_DIET_MIN_B", "1"}}},
    {"dietmin1000000", {{"SCTC_CTC_DIET_MIN_B", "1000000"}}},
    {"diag1", {{"SCTC_CTC_DIAG", "1"}}},
    {"diag2", {{"SCTC_CTC_DIAG", "2"}}},
    {"diag6", {{"SCTC_CTC_DIAG", "6"}}},
    {"diag8", {{"SCTC_CTC_DIAG", "8"}}},
    {"diag14", {{"SCTC_CTC_DIAG", "14"}}},
    // the combinations of tests/test_gpu_ctc_paths.py (path.ENV), tests/test_abi.py and tools/ctc_*.py
    {"helper0+dietmin1", {{"SCTC_CTC_HELPER", "0"}, {"SCTC_CTC_DIET_MIN_B", "1"}}},
    {"helper0+dietmin1000000", {{"SCTC_CTC_HELPER", "0"}, {"SCTC_CTC_DIET_MIN_B", "1000000"}}},
    {"helper0+diag1", {{"SCTC_CTC_HELPER", "0"}, {"SCTC_CTC_DIAG", "1"}}},
    {"wide1+waves8", {{"SCTC_CTC_WIDE", "1"}, {"SCTC_CTC_WAVES", "8"}}},
    {"wide1+store64", {{"SCTC_CTC_WIDE", "1"}, {"SCTC_CTC_STORE", "64"}}},
    {"widemin1+store64", {{"SCTC_CTC_WIDE_MIN_B", "1"}, {"SCTC_CTC_STORE", "64"}}},
    {"wide0+fused0", {{"SCTC_CTC_WIDE", "0"}, {"SCTC_CTC_FUSED", "0"}}},
    // the lattice kernel's forced shapes
    {"fused0+waves1", {{"SCTC_CTC_FUSED", "0"}, {"SCTC_CTC_WAVES", "1"}}},
    {"fused0+waves4", {{"SCTC_CTC_FUSED", "0"}, {"SCTC_CTC_WAVES", "4"}}},
    {"fused0+waves8", {{"SCTC_CTC_FUSED", "0"}, {"SCTC_CTC_WAVES", "8"}}},
    {"lazy+waves4", {{"SCTC_CTC_LAZY", "1"}, {"SCTC_CTC_WAVES", "4"}}},
};
static const char* const SWITCH_NAMES[] = {"SCTC_CTC_GENERIC", "SCTC_CTC_LAZY", "SCTC_CTC_FUSED", "SCTC_CTC_STORE", "SCTC_CTC_WIDE",
                                           "SCTC_CTC_WIDE_MIN_B", "SCTC_CTC_WAVES", "SCTC_CTC_HELPER", "SCTC_CTC_HELPER_MAX_B",
                                           "SCTC_CTC_DIET_MIN_B", "SCTC_CTC_DIAG"};
static void apply(const SwitchSet& s)
{
    for (const char* n : SWITCH_NAMES) unsetenv(n);
    for (const auto& kv : s.env) if (kv[0]) setenv(kv[0], kv[1], 1);
}

// rows of 2U+1 states on both sides of 128, 256, 512, 1024 and 2048 (the last: the generic kernels), and the shortest row
static const int GRID_U[] = {1, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024};
// utterances on both sides of 18, 24 (the wide kernel), 256 (helper waves) and 1025 (the diet)
static const int GRID_B[] = {1, 17, 18, 23, 24, 256, 257, 1024, 1025};
static const int GRID_A[] = {64, 65, 128, 129, 256, 257};

// ragged batches: {T, U} per utterance
struct Batch { const char* name; int A, B; int tu[25][2]; };
static const Batch BATCHES[] = {
    {"narrow", 33, 7, {{5, 3}, {40, 17}, {100, 255}, {1, 1}, {33, 64}, {77, 128}, {250, 100}}},
    {"wide", 20, 25, {{700, 300}, {461, 401}, {900, 600}, {333, 257}, {1024, 1023}, {17, 5}, {650, 512}, {512, 511}, {801, 400},
                      {390, 333}, {999, 999}, {1, 1}, {720, 360}, {1300, 650}, {555, 444}, {345, 300}, {876, 543}, {1000, 500},
                      {432, 321}, {610, 600}, {777, 388}, {1201, 600}, {680, 340}, {404, 303}, {963, 852}}},
    {"long", 70, 5, {{1200, 1100}, {800, 30}, {2300, 1024}, {64, 63}, {3, 1}}},
};

static void print_kernels(const CtcPlan& p, const CtcLayout* lay)
{
    char names[2][96];
    const int n = ctc_plan_kernel_name(p, names);
    for (int i = 0; i < n; ++i) {
        printf(" %s\n", names[i]);
        if (lay && i == 0)
            printf(" utts %zu labels %zu store %zu sync %zu ll %zu skip2 %zu alpha %zu beta %zu scratch %zu\n", lay->utts, lay->labels,
                   lay->store, lay->sync, lay->ll, lay->skip2, lay->alpha, lay->beta, lay->scratch);
    }
}

static void grid()
{
    for (int U : GRID_U) for (int B : GRID_B) for (int A : GRID_A) for (int dtype = 0; dtype < 2; ++dtype)
        for (const SwitchSet& s : SETS) {
            apply(s);
            printf("plan %d %d %d %d %s\n", 2 * U + 1, B, A, dtype, s.name);
            print_kernels(ctc_plan({B, A, dtype, 2 * U + 1, 1}, ctc_switches_from_env()), nullptr);
        }
    for (const Batch& bt : BATCHES) for (int dtype = 0; dtype < 2; ++dtype)
        for (const SwitchSet& s : SETS) {
            apply(s);
            printf("layout %s %d %s\n", bt.name, dtype, s.name);
            std::vector<int32_t> T(bt.B), U(bt.B);
            int max_L = 0, max_T = 0;
            for (int b = 0; b < bt.B; ++b) {
                T[b] = bt.tu[b][0];
                U[b] = bt.tu[b][1];
                if (2 * U[b] + 1 > max_L) max_L = 2 * U[b] + 1;
                if (T[b] > max_T) max_T = T[b];
            }
            const CtcPlan p = ctc_plan({bt.B, bt.A, dtype, max_L, max_T}, ctc_switches_from_env());
            std::vector<CtcUtt> utts(bt.B);
            const CtcLayout lay = ctc_layout(p, T.data(), U.data(), utts.data());
            printf(" lat_off");
            for (const CtcUtt& u : utts) printf(" %lld", (long long)u.lat_off);
            printf("\n");
            print_kernels(p, &lay);
            printf(" bytes %zu\n", lay.bytes);
        }
}

static void query()
{
    const CtcSwitches sw = ctc_switches_from_env();
    CtcShape s;
    while (scanf("%d %d %d %d %d", &s.B, &s.A, &s.dtype, &s.max_L, &s.max_T) == 5) {
        print_kernels(ctc_plan(s, sw), nullptr);
        printf("end\n");
    }
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "grid")) grid();
    else if (argc == 2 && !strcmp(argv[1], "query")) query();
    else return 2;
    return 0;
}
