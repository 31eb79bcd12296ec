// Prints the decisions of csrc/lm_score_plan.h (tests/test_lm_score_plan_cpu.py compiles this with g++).
//   stdin: lines "kind A tile_bytes terms_in_ws N U_0 .. U_{N-1}"; label_off[n] = 1000 * n
//   per line: "plan n_terms n_tiles resident grid", "off seqs tiles sym terms scratch bytes",
//             "seq n U term_off label_off" per descriptor in the plan's order, "tile first cnt steps" per tile, "end"
#include <stdio.h>

#include <vector>

#include "lm_score_plan.h"

using namespace sctc;

int main()
{
    int kind, A, terms_in_ws, N;
    unsigned long long tile_bytes;
    while (scanf("%d %d %llu %d %d", &kind, &A, &tile_bytes, &terms_in_ws, &N) == 5) {
        std::vector<int32_t> U(N);
        std::vector<int64_t> off(N);
        for (int n = 0; n < N; ++n) {
            if (scanf("%d", &U[n]) != 1) return 2;
            off[n] = 1000ll * n;
        }
        const LmScorePlan p = lm_score_plan(kind, N, A, U.data(), off.data(), (size_t)tile_bytes, terms_in_ws != 0);
        printf("plan %lld %lld %d %d\n", (long long)p.n_terms, (long long)p.n_tiles, p.resident, p.grid);
        printf("off %zu %zu %zu %zu %zu %zu\n", p.off_seqs, p.off_tiles, p.off_sym, p.off_terms, p.off_scratch, p.bytes);
        for (const LmSeq& s : p.seqs) printf("seq %d %d %lld %lld\n", s.n, s.U, (long long)s.term_off, (long long)s.label_off);
        for (const LmTile& t : p.tiles) printf("tile %d %d %d\n", t.first, t.cnt, t.steps);
        printf("end\n");
    }
    return 0;
}
