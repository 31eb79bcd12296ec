// Replays the delta-buffer route of csrc/bwd_overlap_plan.h on real memory, host only: every buffer is an array of its
// own, every GEMM of the pass a function that reads and writes whole arrays, run in the engine's launch order
// (tests/test_bwd_overlap_plan_cpu.py builds this with -fsanitize=address,undefined and runs it).  For NL in 1..7 x TL in
// 0..NL, serial and overlap order: bwd_route_check accepts the route, no index leaves its array, and every weight
// gradient sees exactly the delta that the serial order gives it -- the deferred ones although they run behind every delta
// GEMM in front of the join.  Exit status 0 and "ok N routes", or 1 and the first difference.
#include <stdio.h>

#include <vector>

#include "bwd_overlap_plan.h"

using namespace sctc;

static constexpr int W = 8;    // elements per buffer

struct Pass {
    int NL, TL;
    bool overlap;
    BwdRoute r;
    std::vector<std::vector<long>> buf;     // [BwdBuf]
    std::vector<unsigned long long> seen;   // [loop index]: checksum of what dW_i read

    std::vector<long>& at(int b) { return buf.at((size_t)b); }
    void wgrad(int i)
    {
        unsigned long long s = 0;
        for (long v : at(r.d_in[i])) s = s * 31u + (unsigned long long)v;
        seen.at((size_t)i) = s;
    }
    void delta(int i)       // d_out_i = f_i(d_in_i)
    {
        const std::vector<long> in = at(r.d_in[i]);
        std::vector<long>& out = at(r.d_out[i]);
        for (int k = 0; k < W; ++k) out.at((size_t)k) = in.at((size_t)k) * 7 + i + 1;
    }
    bool run()
    {
        if (!bwd_route(NL, TL, overlap, &r)) return false;
        const int extra = overlap ? bwd_overlap_hh_above(NL, TL) - 1 : 0;
        buf.assign((size_t)(BWD_BUF_X0 + extra), std::vector<long>(W, 0));     // exactly the buffers the engine carves
        for (int k = 0; k < W; ++k) at(BWD_BUF_LOGITS).at((size_t)k) = 1000 + k;
        seen.assign((size_t)NL + 1, 0);
        if (overlap) {
            for (int i = NL; i >= TL; --i) delta(i);        // in front of the BPTT grid
            for (int i = NL; i >= TL; --i) wgrad(i);        // beside it
        }
        for (int i = overlap ? TL - 1 : NL; i >= 0; --i) {
            wgrad(i);
            if (i >= 1) delta(i);
        }
        return true;
    }
};

int main()
{
    int n = 0;
    for (int NL = 1; NL <= 7; ++NL)
        for (int TL = 0; TL <= NL; ++TL) {
            Pass serial = {NL, TL, false, {}, {}, {}};
            if (!serial.run() || bwd_route_check(NL, TL, false, serial.r) != 0) {
                printf("NL %d TL %d: the serial route fails its check\n", NL, TL);
                return 1;
            }
            ++n;
            const bool can = bwd_overlap_config_ok(NL, TL, 1824, true, true);
            Pass ov = {NL, TL, true, {}, {}, {}};
            if (!can) {
                if (bwd_overlap_hh_above(NL, TL) < 2 && bwd_route(NL, TL, true, &ov.r)) {
                    printf("NL %d TL %d: an overlap route where there is nothing to overlap\n", NL, TL);
                    return 1;
                }
                continue;
            }
            if (!ov.run() || bwd_route_check(NL, TL, true, ov.r) != 0) {
                printf("NL %d TL %d: the overlap route fails its check\n", NL, TL);
                return 1;
            }
            for (int i = 0; i <= NL; ++i) {
                if (ov.r.deferred[i] != (i >= TL)) { printf("NL %d TL %d: loop index %d deferred wrongly\n", NL, TL, i); return 1; }
                if (ov.seen[(size_t)i] != serial.seen[(size_t)i]) {
                    printf("NL %d TL %d: dW of loop index %d reads another delta than in the serial order\n", NL, TL, i);
                    return 1;
                }
            }
            ++n;
        }
    printf("ok %d routes\n", n);
    return 0;
}
