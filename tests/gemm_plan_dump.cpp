// Prints the decisions of csrc/gemm_plan.h for tests/test_gemm_plan_cpu.py (host only, g++).
//   gemm_plan_dump queries   the (query, setting) pairs of the recorded table, one per line
//   gemm_plan_dump grid      the same lines, each followed by " | " and the decision
//   gemm_plan_dump plan      stdin: lines "M N K akc bkc gather a2 prec in16" -> the decision under the environment
//   gemm_plan_dump sizing    every launch the engine can make against the workspace its create-time rule sizes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "gemm_plan.h"

using namespace sctc;

struct Q { int M, N, K, akc, bkc, gather, a2, prec, in16; };

static GemmQuery query_of(const Q& c)
{
    GemmQuery q{c.M, c.N, c.K, c.prec, c.in16, c.akc, c.bkc};
    q.idx_a = c.gather && !c.akc;     // the recurrent weight gradient gathers both operands
    q.idx_b = c.gather && !c.bkc;
    q.a2 = c.a2 != 0;
    return q;
}

// "S1T0": SCTC_GEMM_SHAPE=1 SCTC_H16_TILE=0; "G0": SCTC_G16=0; "default": none of the three
static void apply_setting(const char* name)
{
    unsetenv("SCTC_GEMM_SHAPE");
    unsetenv("SCTC_H16_TILE");
    unsetenv("SCTC_G16");
    if (!strcmp(name, "default")) return;
    for (const char* p = name; *p; p += 2) {
        const char v[2] = {p[1], 0};
        setenv(*p == 'S' ? "SCTC_GEMM_SHAPE" : (*p == 'T' ? "SCTC_H16_TILE" : "SCTC_G16"), v, 1);
    }
}

static std::string kernel_name(const GemmPlan& p)
{
    char b[96];
    const auto tf = [](bool v) { return v ? "true" : "false"; };
    switch (p.kernel) {
        case GEMM_F32: snprintf(b, sizeof(b), "gemm_f32_kernel<%s, %s, %d, %s>", tf(p.ak), tf(p.bkc), p.shape, tf(p.a2)); break;
        case GEMM_H16: snprintf(b, sizeof(b), "gemm_h16_kernel<%s, %s, %s, %d>", tf(p.ak), tf(p.bkc), tf(p.bf), (int)p.big); break;
        case GEMM_X16: snprintf(b, sizeof(b), "gemm_x16_kernel<%s, %s, %d>", tf(p.ak), tf(p.bf), (int)p.big); break;
        case GEMM_G16: snprintf(b, sizeof(b), "gemm_g16_kernel<%s, %s>", tf(p.ak), tf(p.bf)); break;
        default: snprintf(b, sizeof(b), "gemm_s3_kernel<%s, %s, %s>", tf(p.ak), tf(p.bkc), tf(p.gather && !(p.ak && p.bkc))); break;
    }
    return b;
}

static void print_query(const Q& c) { printf("q %d %d %d %d %d %d %d %d %d", c.M, c.N, c.K, c.akc, c.bkc, c.gather, c.a2, c.prec, c.in16); }

// what launch_gemm_f32 launches for the query (or why not), then what the planner proposes
static void print_decision(const Q& c)
{
    const GemmQuery q = query_of(c);
    const GemmPlan p = gemm_plan(q, gemm_switches_from_env());
    char why[160];
    if (gemm_validate(q, why, sizeof(why))) printf("%s block %d lds %d grid %d", kernel_name(p).c_str(), p.threads, p.lds_bytes, p.grid_x);
    else printf("rejected: %s", why);
    printf(" | splits %d ws %lld\n", p.splits, (long long)p.ws_floats);
}

// ---------------------------------------------------------------- the engine's GEMMs (brnn_engine.hip)

struct Net { int D, A, H, NL, TL; int dtype; };     // dtype: 0 fp32, 1 "fp16 activations", 3 bf16x3
static int pad32(int v) { return (v + 31) / 32 * 32; }

// run_forward / run_backward for a minibatch of N frames whose recurrent weight gradients pair K rows
static void engine_queries(const Net& n, int N, int K, std::vector<Q>* out)
{
    const int Dp = pad32(n.D), Hp = pad32(n.H), Ap = pad32(n.A);
    const int in16 = n.dtype == 1, fwd = n.dtype == 1 ? 1 : n.dtype, bwd = n.dtype == 1 ? 2 : n.dtype;
    for (int l = 0; l <= n.NL; ++l) {
        const int inp = l == 0 ? Dp : Hp, outp = l == n.NL ? Ap : Hp;
        out->push_back({N, outp, inp, 1, 1, 0, n.dtype == 0 && n.TL > 0 && l == n.TL, fwd, in16});            // forward
        out->push_back({outp, inp, N, 0, 0, 0, n.dtype == 0 && n.TL > 0 && l == n.TL - 1, bwd, in16});        // weight gradient
        if (l > 0) out->push_back({N, inp, outp, 1, in16, 0, 0, bwd, in16});                                    // delta
    }
    if (n.TL > 0)
        for (int gather = 0; gather < 2; ++gather) out->push_back({Hp, Hp, K, 0, 0, gather, 0, bwd, in16});    // recurrent weight gradients
}

static const Net CONFIGS[5] = {{615, 28, 512, 2, 1, 0}, {943, 62, 1024, 3, 2, 0}, {483, 33, 1824, 5, 3, 0},
                               {615, 33, 1824, 5, 3, 0}, {615, 33, 2048, 7, 4, 1}};
static const int CONFIG_FRAMES[5] = {200, 300, 32000, 64000, 64000}, CONFIG_UTTS[5] = {1, 1, 32, 32, 8};

// ---------------------------------------------------------------- the recorded table's queries

static const char* const SETS_ALL[] = {"default", "S0", "S1", "S2", "S3", "T0", "T1", "G0", "S0T0", "S1T0", "S2T0", "S3T0", "S0T1",
                                       "S1T1", "S2T1", "S3T1", "S0G0", "S1G0", "S2G0", "S3G0", "T0G0", "T1G0", nullptr};
static const char* const SETS_F32[] = {"default", "S0", "S1", "S2", "S3", nullptr};
static const char* const SETS_16[] = {"default", "T0", "T1", "G0", "T0G0", "T1G0", nullptr};
static const char* const SETS_NONE[] = {"default", nullptr};

static const char* const* sets_of(const Q& c) { return c.prec == 0 ? SETS_F32 : (c.prec == 3 ? SETS_NONE : SETS_16); }

template <typename F>
static void for_each_pair(F visit)
{
    std::set<std::vector<int>> seen;      // the sections overlap in a few queries
    const auto f = [&](const Q& c, const char* const* sets) {
        if (seen.insert({c.M, c.N, c.K, c.akc, c.bkc, c.gather, c.a2, c.prec, c.in16}).second) visit(c, sets);
    };
    // every layout, gather, A2 and precision (illegal combinations included) under every setting
    const int cross[4][3] = {{132, 132, 520}, {2052, 2052, 4104}, {1824, 1824, 32000}, {264, 136, 4096}};
    const int precs[8][2] = {{0, 0}, {1, 0}, {2, 0}, {1, 1}, {2, 1}, {3, 0}, {0, 1}, {3, 1}};
    for (const auto& s : cross)
        for (int lay = 0; lay < 4; ++lay)
            for (int gather = 0; gather < (lay == 3 ? 1 : 2); ++gather)
                for (int a2 = 0; a2 < 2; ++a2)
                    for (const auto& pr : precs) f(Q{s[0], s[1], s[2], lay & 1, lay >> 1, gather, a2, pr[0], pr[1]}, SETS_ALL);
    // fp32 / rounding in registers / 16-bit in memory K-contiguous, row-contiguous (M % 8 == 4 included), gathered / bf16x3
    const Q variants[6] = {{0, 0, 0, 1, 1, 0, 0, 0, 0}, {0, 0, 0, 1, 1, 0, 0, 1, 0}, {0, 0, 0, 1, 1, 0, 0, 2, 1},
                           {0, 0, 0, 0, 0, 0, 0, 2, 1}, {0, 0, 0, 0, 0, 1, 0, 2, 1}, {0, 0, 0, 0, 0, 0, 0, 3, 0}};
    const auto shape = [&](int M, int N, int K, bool mem16_only) {
        for (const Q& v : variants) {
            if (mem16_only && !v.in16) continue;
            Q c = v;
            c.M = M; c.N = N; c.K = K;
            f(c, sets_of(c));
        }
    };
    // M and N on both sides of one and two multiples of 64 / 96 / 128 / 256
    const int edge[18] = {60, 64, 68, 92, 96, 100, 124, 128, 132, 188, 192, 196, 252, 256, 260, 508, 512, 516};
    const int other[6] = {64, 100, 128, 192, 260, 512};
    for (int swap = 0; swap < 2; ++swap)
        for (int e : edge)
            for (int o : other) {
                shape(swap ? o : e, swap ? e : o, 1032, false);
                shape(swap ? o : e, swap ? e : o, 4096, true);
            }
    // K on both sides of 8 and 64 K tiles (of 16 and of 64) and of 4096, on outputs on both sides of the tile-count
    // thresholds: 8 and 32 tiles of 256, two rounds of resident blocks, the 6 % and 25 % padding allowances
    const int ks[12] = {120, 128, 136, 504, 512, 520, 1016, 1024, 1032, 4088, 4096, 4104};
    const int outs[21][2] = {{132, 132}, {1824, 1824}, {2048, 640}, {1792, 256}, {2048, 256}, {7936, 256}, {8192, 256}, {6016, 4096},
                             {6144, 4096}, {4096, 4096}, {5888, 5632}, {6144, 5632}, {1160, 1160}, {1096, 2052}, {260, 2048},
                             {3900, 4096}, {3840, 3840}, {128, 3744}, {576, 128}, {128, 576}, {128, 704}};
    for (const auto& o : outs)
        for (int k : ks) shape(o[0], o[1], k, false);
    // every GEMM of the five BASELINE.json configurations at their own minibatch sizes
    for (int i = 0; i < 5; ++i) {
        std::vector<Q> qs;
        engine_queries(CONFIGS[i], CONFIG_FRAMES[i], CONFIG_FRAMES[i] - CONFIG_UTTS[i], &qs);
        for (const Q& c : qs) f(c, sets_of(c));
    }
}

// ---------------------------------------------------------------- the sizing sweep

// every N in 1..F next to a multiple of 16 (every K-tile edge of every kernel), 1..64, around 4096, and F
static std::vector<int> frames_upto(int F)
{
    std::set<int> s = {F};
    for (int n = 1; n <= 64 && n <= F; ++n) s.insert(n);
    for (int m = 16; m <= F + 1; m += 16)
        for (int n = m - 1; n <= m + 1; ++n)
            if (n <= F) s.insert(n);
    return std::vector<int>(s.begin(), s.end());
}

// Returns the plans that do not fit and should: every weight-gradient plan (those launches took the planned split
// unchecked before there was one helper), and every forward / delta plan up to the cap.  *capped: forward / delta plans
// above the cap, which run unsplit by design.
static int check_sizing(const Net& n, int F, long long* checked, long long* capped)
{
    const GemmSwitches sw = gemm_switches_from_env();
    const int Dp = pad32(n.D), Hp = pad32(n.H), Ap = pad32(n.A);
    const int64_t have = brnn_splitk_floats(Dp, Hp, Ap, n.NL, n.TL > 0, F, true, n.dtype == 1 ? 2 : n.dtype, n.dtype == 1, sw);
    int bad = 0;
    for (int N : frames_upto(F))
        for (int K : {N - 1, N - 2, N / 2}) {      // pairs: frames - utterances
            if (K < 0) continue;
            std::vector<Q> qs;
            engine_queries(n, N, K, &qs);
            for (const Q& c : qs) {
                const GemmPlan p = gemm_plan(query_of(c), sw);
                ++*checked;
                if (p.ws_floats <= have) continue;
                if (c.akc && p.ws_floats > BRNN_SPLITK_CAP) { ++*capped; continue; }     // forward / delta (A K-contiguous)
                if (bad++ < 20) {
                    printf("uncovered: D %d H %d A %d dtype %d F %d have %lld: ", n.D, n.H, n.A, n.dtype, F, (long long)have);
                    print_query(c);
                    printf(" needs %lld (%d splits)\n", (long long)p.ws_floats, p.splits);
                }
            }
        }
    return bad;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "queries" || mode == "grid") {
        for_each_pair([&](const Q& c, const char* const* sets) {
            for (; *sets; ++sets) {
                print_query(c);
                printf(" %s", *sets);
                if (mode == "grid") {
                    apply_setting(*sets);
                    printf(" | ");
                    print_decision(c);
                } else {
                    printf("\n");
                }
            }
        });
        return 0;
    }
    if (mode == "plan") {
        Q c;
        while (scanf("%d %d %d %d %d %d %d %d %d", &c.M, &c.N, &c.K, &c.akc, &c.bkc, &c.gather, &c.a2, &c.prec, &c.in16) == 9) {
            const GemmPlan p = gemm_plan(query_of(c), gemm_switches_from_env());
            printf("%d %d %d %d\n", p.bm, p.bn, p.bk, (int)p.split_tile_differs);
        }
        return 0;
    }
    if (mode == "sizing") {
        long long checked = 0, capped = 0;
        int bad = 0;
        for (int dtype : {0, 1, 3}) {
            for (int i = 0; i < 5; ++i) {
                Net n = CONFIGS[i];
                n.dtype = dtype;
                bad += check_sizing(n, CONFIG_FRAMES[i], &checked, &capped);
            }
            const int dims[5] = {32, 64, 288, 1824, 2048};
            for (int D : dims)
                for (int H : dims)
                    for (int A : dims)
                        for (int F : {8, 100, 1000, 5000}) bad += check_sizing(Net{D, A, H, 2, 1, dtype}, F, &checked, &capped);
        }
        printf("%lld plans checked, %lld forward / delta plans above the cap, %d uncovered\n", checked, capped, bad);
        return bad ? 1 : 0;
    }
    fprintf(stderr, "usage: gemm_plan_dump queries | grid | plan | sizing\n");
    return 2;
}
