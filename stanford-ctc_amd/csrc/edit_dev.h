// Device code that the edit-distance kernels share (edit_distance.hip, nbest_mbr.hip): the wavefront of one pair,
// DESIGN.md §4.8, once.  Device only.
//
// One wave per pair.  A lane owns CPL = 4 consecutive columns of b; a panel is the 256 columns of the 64 lanes.  The
// wave walks the rows of a skewed by one row per lane: at step s lane l computes row s - l of its columns, takes the
// right-edge cell of lane l - 1 for that row with one cross-lane shift (xlane.h) and keeps its own previous row in
// registers.  The symbol of the row travels down the lanes the same way.  A pair with more than 256 columns is walked
// panel by panel; the right edge of a panel (all n rows) waits in LDS for the next.
//
// A cell carries (D, up, left): the distance and two of the four counts of the path that the trace-back of the
// reference would take from that cell (the first of MATCH / UP / LEFT / SUB that holds, editDistance.py:29-38).  The
// other two follow from i = up + sub + match and D = up + left + sub, so the counts need neither a stored table nor a
// trace-back.  Only the alignment does: with OPS every cell's 2-bit operation is stored (16 cells = 4 rows x 4 columns
// of one lane per 32-bit word, in LDS when the pair fits, in the caller's workspace otherwise) and one lane walks back
// from (n, m).  The length of the path is D + match, known before the walk, so the codes are written in forward order
// straight away.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xlane.h"

namespace sctc {
namespace {

constexpr int EDIT_MAX_LEN = 8191;      // D, up and left fit 13 bits
constexpr int CPL = 4;                  // columns per lane
constexpr int PANEL = 64 * CPL;         // columns per panel
constexpr int WAVES = 4;                // waves (pairs) per workgroup of the common launch
constexpr size_t SLOT_MAX = 16384;      // LDS bytes of one wave in the four-wave launch (64 KB per workgroup)

enum : int { OP_MATCH = 0, OP_UP = 1, OP_LEFT = 2, OP_SUB = 3 };

struct EditPair {
    int64_t a_off, b_off;   // elements
    int64_t ops_off;        // bytes into ops_dev
    int64_t tab_off;        // bytes into the workspace: the operation table when it is not in LDS
    int32_t n, m;
    int32_t p;              // index of the pair in the caller's order
    int32_t lds_tab;        // the operation table lives in the wave's LDS slot, behind the panel edge
};

struct EditArgs {
    const EditPair* pairs;  // pinned host memory, read once per wave
    int32_t count;
    int32_t slot;           // LDS bytes per wave
    const int32_t* a;
    const int32_t* b;
    int32_t* stats;
    int8_t* ops;
    int32_t* ops_len;
    char* ws;
};

__device__ __forceinline__ int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

template <bool OPS>
__device__ __forceinline__ void edit_pair(const EditArgs& p, const EditPair& d, char* slot, const int lane)
{
    const int n = d.n, m = d.m;
    const int32_t* a = p.a + d.a_off;
    const int32_t* b = p.b + d.b_off;
    int32_t* st = p.stats + 5 * (int64_t)d.p;
    int8_t* ops = OPS ? p.ops + d.ops_off : nullptr;
    if (n == 0 || m == 0) {     // the leftover rule alone (editDistance.py:42-43): n UPs or m LEFTs
        if (lane == 0) {
            st[0] = n + m; st[1] = n; st[2] = m; st[3] = 0; st[4] = 0;
            if (OPS) p.ops_len[d.p] = n + m;
        }
        if (OPS)
            for (int k = lane; k < n + m; k += 64) ops[k] = n ? OP_UP : OP_LEFT;
        return;
    }
    int2* edge = (int2*)slot;                               // [n] right edge of the previous panel: (D, up | left << 16)
    const int tstride = (m + CPL - 1) / CPL;                // words per group of four rows
    uint32_t* tab = nullptr;
    if (OPS) tab = d.lds_tab ? (uint32_t*)(slot + (m > PANEL ? (size_t)n * sizeof(int2) : 0)) : (uint32_t*)(p.ws + d.tab_off);

    int fd = 0, fc = 0;                                     // cell (n, m)
    for (int pbase = 0; pbase < m; pbase += PANEL) {
        const int pw = min(PANEL, m - pbase);
        const int nl = (pw + CPL - 1) / CPL;                // lanes that own a column
        const bool last = pbase + PANEL >= m;
        const int col0 = pbase + lane * CPL;
        int bj[CPL], pd[CPL], pc[CPL];                      // my symbols of b, my cells of the previous row
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int col = col0 + k;
            bj[k] = col < m ? b[col] : 0;
            pd[k] = col + 1;                                // D[0, j] = j, all LEFT
            pc[k] = (col + 1) << 16;
        }
        int dd = col0, dc = col0 << 16;                     // D[0, col0]: the diagonal neighbour of my first cell
        int od = 0, oc = 0, asym = 0;                       // my right-edge cell of the last row, its symbol of a
        int abuf = 0, ed = 0, ec = 0;                       // 64 rows of a and of the panel's left edge, one per lane
        uint32_t opw = 0;
        const int steps = n + nl - 1;
        for (int s = 0; s < steps; ++s) {
            if ((s & 63) == 0) {
                const int r0 = s + lane, rr = min(r0, n - 1);
                abuf = a[rr];
                if (pbase == 0) {
                    ed = r0 + 1;                            // D[i, 0] = i, all UP
                    ec = r0 + 1;
                } else {
                    const int2 e = edge[rr];
                    ed = e.x;
                    ec = e.y;
                }
            }
            int rd = lane_shr1(od), rc = lane_shr1(oc), as = lane_shr1(asym);
            const int sl = s & 63;
            const int hd = rdlane(ed, sl), hc = rdlane(ec, sl), ha = rdlane(abuf, sl);
            if (lane == 0) { rd = hd; rc = hc; as = ha; }
            asym = as;
            const int r = s - lane;                         // my row of this step
            if (r >= 0 && r < n) {
                int ld = rd, lc = rc, gd = dd, gc = dc;     // left and diagonal neighbours
                uint32_t opb = 0;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int ud = pd[k], uc = pc[k];
                    const int mn = min(ud, min(ld, gd));
                    int nd, nc, op;
                    if (asym == bj[k]) { nd = gd; nc = gc; op = OP_MATCH; }
                    else if (ud == mn) { nd = mn + 1; nc = uc + 1; op = OP_UP; }
                    else if (ld == mn) { nd = mn + 1; nc = lc + 0x10000; op = OP_LEFT; }
                    else { nd = mn + 1; nc = gc; op = OP_SUB; }
                    gd = ud; gc = uc;
                    ld = nd; lc = nc;
                    pd[k] = nd; pc[k] = nc;
                    if (OPS) opb |= (uint32_t)op << (2 * k);
                }
                dd = rd; dc = rc;
                od = pd[CPL - 1]; oc = pc[CPL - 1];
                if (!last && lane == 63) edge[r] = make_int2(od, oc);
                if (OPS) {
                    opw |= opb << (8 * (r & 3));
                    if ((r & 3) == 3 || r == n - 1) {
                        if (lane < nl) tab[(size_t)(r >> 2) * tstride + (pbase / CPL) + lane] = opw;
                        opw = 0;
                    }
                }
            }
        }
        if (last) {
            const int lf = (m - 1 - pbase) / CPL, kf = (m - 1 - pbase) % CPL;
            int vd = pd[0], vc = pc[0];
#pragma unroll
            for (int k = 1; k < CPL; ++k)
                if (kf == k) { vd = pd[k]; vc = pc[k]; }
            fd = rdlane(vd, lf);
            fc = rdlane(vc, lf);
        } else {
            // lane 63 wrote the edge, every lane of the next panel reads it: same wave, so a fence and a
            // wave barrier order the two without a workgroup barrier
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
    const int up = fc & 0xffff, left = fc >> 16, sub = fd - up - left, match = n - up - sub;
    if (lane == 0) { st[0] = fd; st[1] = up; st[2] = left; st[3] = sub; st[4] = match; }
    if (!OPS) return;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the table was written by every lane of this wave
    if (lane == 0) {
        const int len = max(0, min(fd + match, n + m));    // D + match operations; never beyond the pair's share of ops
        p.ops_len[d.p] = len;
        int i = n, j = m, pos = len - 1;
        while (i > 0 && j > 0 && pos >= 0) {                // editDistance.py:28-40, editDist.pyx:69-93
            const uint32_t w = tab[(size_t)((i - 1) >> 2) * tstride + ((j - 1) >> 2)];
            const int op = (w >> (8 * ((i - 1) & 3) + 2 * ((j - 1) & 3))) & 3;
            ops[pos--] = (int8_t)op;
            i -= op != OP_LEFT;
            j -= op != OP_UP;
        }
        for (; i > 0 && pos >= 0; --i) ops[pos--] = OP_UP;  // editDistance.py:42-43, editDist.pyx:94-106
        for (; j > 0 && pos >= 0; --j) ops[pos--] = OP_LEFT;
    }
}

}  // namespace
}  // namespace sctc
