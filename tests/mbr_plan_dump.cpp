// Prints the decisions of csrc/nbest_mbr_plan.h (tests/test_mbr_plan_cpu.py compiles this with g++).
//   stdin: lines "intern N G U_0 .. U_{N-1} g_0 .. g_G" or "mbr B K unit flags Kb_0 .. Kb_{B-1} U_0 .. U_{B*K-1}";
//          label_off[n] = 1000 * n
//   intern: "slots n_slots n_table", "off rows groups head base meta table fill bytes",
//           "row n U label_off slot_off tab_off tab_mask" per row, "group first end" per group, "end"
//   mbr:    "plan n_common pairs_common pairs_alone slot_common slot_alone cslot_common cslot_alone tab_stride conf_slots",
//           "off rows utts kb lens head status ids intern dist w z match ops tab bytes",
//           "utt b kb pair_off conf_off longest" per utterance in the plan's order, "row o row_off bound" per row, "end"
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nbest_mbr_plan.h"

using namespace sctc;

int main()
{
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "intern")) {
            int N, G;
            if (scanf("%d %d", &N, &G) != 2) return 2;
            std::vector<int32_t> U(N), g(G + 1);
            std::vector<int64_t> off(N);
            for (int n = 0; n < N; ++n) {
                if (scanf("%d", &U[n]) != 1) return 2;
                off[n] = 1000ll * n;
            }
            for (int i = 0; i <= G; ++i)
                if (scanf("%d", &g[i]) != 1) return 2;
            const InternPlan p = intern_plan(N, U.data(), off.data(), G, g.data());
            printf("slots %lld %lld\n", (long long)p.n_slots, (long long)p.n_table);
            printf("off %zu %zu %zu %zu %zu %zu %zu %zu\n", p.off_rows, p.off_groups, p.head_bytes, p.off_base, p.off_meta,
                   p.off_table, p.fill_bytes, p.bytes);
            for (int n = 0; n < N; ++n)
                printf("row %d %d %lld %lld %lld %u\n", n, p.rows[n].U, (long long)p.rows[n].label_off, (long long)p.rows[n].slot_off,
                       (long long)p.rows[n].tab_off, p.rows[n].tab_mask);
            for (const InternGroup& q : p.groups) printf("group %d %d\n", q.first, q.end);
        } else if (!strcmp(what, "mbr")) {
            int B, K, unit, flags;
            if (scanf("%d %d %d %d", &B, &K, &unit, &flags) != 4) return 2;
            std::vector<int32_t> Kb(B), U((size_t)B * K);
            std::vector<int64_t> off((size_t)B * K);
            for (int b = 0; b < B; ++b)
                if (scanf("%d", &Kb[b]) != 1) return 2;
            for (size_t o = 0; o < U.size(); ++o) {
                if (scanf("%d", &U[o]) != 1) return 2;
                off[o] = 1000ll * (long long)o;
            }
            const MbrPlan p = mbr_plan(B, K, unit, flags, Kb.data(), U.data(), off.data());
            printf("plan %d %lld %lld %zu %zu %zu %zu %zu %lld\n", p.n_common, (long long)p.pairs_common, (long long)p.pairs_alone,
                   p.slot_common, p.slot_alone, p.cslot_common, p.cslot_alone, p.tab_stride, (long long)p.conf_slots);
            printf("off %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", p.off_rows, p.off_utts, p.off_kb, p.off_lens,
                   p.head_bytes, p.off_status, p.off_ids, p.off_intern, p.off_dist, p.off_w, p.off_z, p.off_match, p.off_ops,
                   p.off_tab, p.bytes);
            for (const MbrUtt& u : p.utts)
                printf("utt %d %d %lld %lld %d\n", u.b, u.kb, (long long)u.pair_off, (long long)u.conf_off, u.longest);
            for (size_t o = 0; o < U.size(); ++o) printf("row %zu %lld %d\n", o, (long long)p.row_off[o], p.bound[o]);
        } else {
            return 2;
        }
        printf("end\n");
    }
    return 0;
}
