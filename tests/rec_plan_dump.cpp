// Prints the decisions of csrc/recurrent_plan.h (tests/test_recurrence_plan_cpu.py compiles this with g++).
//   rec_plan_dump grid      the grid of tests/data/rec_plan_parent.txt, in its format
//   rec_plan_dump launches  stdin: lines "Hp B prec16 variant cus"; per line the launches of a minibatch of B utterances as
//                           launch_recurrent makes them: "nb FAMILY linear_map name" each, then "end"; "rejected": no such variant
#include <stdio.h>
#include <string.h>

#include "recurrent_plan.h"

using namespace sctc;

static const char* const FAMILY[] = {"Q", "S", "MH", "T", "SLAB", "FALLBACK"};

static void print_plan(int Hp, int B, int prec16, int transpose, int variant, int tcfg, int cus)
{
    RecCandidate c[REC_MAX_CANDIDATES];
    const RecShape s = {Hp, B, prec16, transpose, variant, tcfg, cus};
    const int n = rec_plan(s, c);
    printf("plan %d %d %d %d %d %d %d\n", Hp, B, prec16, transpose, variant, tcfg, cus);
    if (n < 0) printf(" rejected\n");
    for (int i = 0; i < n; ++i) {
        if (c[i].family == REC_FAM_FALLBACK) { printf(" fallback\n"); continue; }
        char name[96];
        rec_candidate_name(c[i], name, sizeof(name));
        printf(" %s %d %zu %d %d %d %d\n", name, c[i].grid, c[i].lds, c[i].per_cu, c[i].fill, c[i].linear_map, c[i].variant);
    }
}

static void print_cuts(int Hp, int B, int prec16, int variant, int cus)
{
    printf("cut %d %d %d %d %d:", Hp, B, prec16, variant, cus);
    for (int b0 = 0; b0 < B;) {
        const RecShape rest = {Hp, B - b0, prec16, 0, variant, 0, cus};
        const int nb = rec_cut(rest);
        printf(" %d", nb);
        b0 += nb;
    }
    printf("\n");
}

static void grid()
{
    static const int HP[] = {96, 512, 1024, 1824, 1856, 2048, 4096};
    static const int BS[] = {1, 3, 4, 5, 6, 8, 16, 17, 32, 33, 64, 65, 96, 128};
    static const int VS[] = {0, 1, 2, 3, 5, 6, 7, 40, 43, 44, 45, 46, 47, 49, 50, 51};
    static const int CB[] = {32, 33, 40, 48, 49, 64, 65, 72, 80, 81, 96, 97, 128, 129, 150, 300};
    static const int CV[] = {0, 1, 40, 45, 47, 50};
    for (int tcfg = 0; tcfg < 4; ++tcfg) {
        for (int Hp : HP) for (int B : BS) {
            if (tcfg == 0) {
                for (int v : VS) for (int p16 = 0; p16 < 2; ++p16) print_plan(Hp, B, p16, 0, v, 0, 256);
                print_plan(Hp, B, 1, 1, 0, 0, 256);
                for (int p16 = 0; p16 < 2; ++p16) print_plan(Hp, B, p16, 0, 0, 0, 32);
            } else {
                for (int p16 = 0; p16 < 2; ++p16) print_plan(Hp, B, p16, 0, 0, tcfg, 256);
            }
        }
        if (tcfg == 0) {
            for (int Hp : HP) for (int B : CB) for (int v : CV) for (int p16 = 0; p16 < 2; ++p16) print_cuts(Hp, B, p16, v, 256);
            for (int Hp : HP) for (int B : CB) for (int p16 = 0; p16 < 2; ++p16) print_cuts(Hp, B, p16, 0, 32);
        }
    }
}

static void launches()
{
    int Hp, B, prec16, variant, cus;
    while (scanf("%d %d %d %d %d", &Hp, &B, &prec16, &variant, &cus) == 5) {
        for (int b0 = 0; b0 < B;) {
            const RecShape rest = {Hp, B - b0, prec16, 0, variant, 0, cus};
            const int nb = rec_cut(rest);
            RecShape one = rest;
            one.B = nb;
            if (one.variant == REC_V_NO_CUT) one.variant = REC_V_AUTO;      // as launch_recurrent hands it on
            RecCandidate c[REC_MAX_CANDIDATES];
            if (rec_plan(one, c) < 0) { printf("rejected\n"); break; }
            char name[96];
            rec_candidate_name(c[0], name, sizeof(name));
            printf("%d %s %d %s\n", nb, FAMILY[c[0].family], c[0].linear_map, name);
            b0 += nb;
        }
        printf("end\n");
    }
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "grid")) grid();
    else if (argc == 2 && !strcmp(argv[1], "launches")) launches();
    else return 2;
    return 0;
}
