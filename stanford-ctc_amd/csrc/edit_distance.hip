// Batched edit distance with error counts and alignments: the Wagner-Fischer table and
// trace-back of ctc_fast/editDistance.py:14-45 (a = ref, b = hyp) and of swbd-utils/editDist.pyx:47-106
// (a = hyp, b = ref) for many pairs of int32 sequences in one launch.
//
// One wave per pair, four waves per workgroup, no communication between waves: edit_pair of edit_dev.h, which
// has the description of the wavefront.  This file plans the pairs (which fit the four-wave launch, whose
// operation table goes to the workspace), stages the descriptors and launches.
#include <algorithm>
#include <vector>

#include "common.h"
#include "edit_dev.h"

namespace sctc {
namespace {

template <bool OPS>
__global__ __launch_bounds__(64 * WAVES) void edit_distance_kernel(EditArgs p)
{
    extern __shared__ __align__(16) char edit_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= p.count) return;                             // whole waves leave; there is no barrier below
    EditPair d = p.pairs[idx];
    d.n = __builtin_amdgcn_readfirstlane(d.n);
    d.m = __builtin_amdgcn_readfirstlane(d.m);
    d.lds_tab = __builtin_amdgcn_readfirstlane(d.lds_tab);
    edit_pair<OPS>(p, d, edit_lds + (size_t)wave * p.slot, lane);
}

struct EditPlan {
    std::vector<EditPair> pairs;    // the four-wave group first, then the pairs that need a workgroup's LDS alone
    int32_t n_common = 0;
    size_t slot_common = 0, slot_alone = 0;
    size_t ws_bytes = 0;
    int64_t ops_total = 0;
    bool any_a = false, any_b = false;
};

int plan_edit(const sctc_edit_config* cfg, EditPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "edit: null config");
    SCTC_CHECK_ARG(cfg->P >= 0, "edit: %d pairs", cfg->P);
    SCTC_CHECK_ARG((cfg->flags & ~SCTC_EDIT_OPS) == 0, "edit: unknown flags 0x%x", cfg->flags);
    if (cfg->P == 0) return SCTC_OK;
    SCTC_CHECK_ARG(cfg->a_len && cfg->a_off && cfg->b_len && cfg->b_off, "edit: null length / offset array");
    const bool want_ops = (cfg->flags & SCTC_EDIT_OPS) != 0;
    std::vector<EditPair> alone;
    pl.pairs.reserve(cfg->P);
    for (int p = 0; p < cfg->P; ++p) {
        const int n = cfg->a_len[p], m = cfg->b_len[p];
        SCTC_CHECK_ARG(n >= 0 && n <= EDIT_MAX_LEN, "edit: pair %d has an a of %d symbols, outside 0..%d", p, n, EDIT_MAX_LEN);
        SCTC_CHECK_ARG(m >= 0 && m <= EDIT_MAX_LEN, "edit: pair %d has a b of %d symbols, outside 0..%d", p, m, EDIT_MAX_LEN);
        SCTC_CHECK_ARG(cfg->a_off[p] >= 0 && cfg->b_off[p] >= 0, "edit: pair %d has a negative offset", p);
        EditPair d{};
        d.a_off = cfg->a_off[p];
        d.b_off = cfg->b_off[p];
        d.ops_off = pl.ops_total;
        d.n = n;
        d.m = m;
        d.p = p;
        pl.ops_total += n + m;
        pl.any_a |= n > 0;
        pl.any_b |= m > 0;
        const bool work = n > 0 && m > 0;
        const size_t edge_b = work && m > PANEL ? (size_t)n * sizeof(int2) : 0;
        const size_t tab_b = work && want_ops ? (size_t)((n + 3) / 4) * ((m + CPL - 1) / CPL) * sizeof(uint32_t) : 0;
        size_t need = edge_b;
        if (tab_b && edge_b + tab_b <= SLOT_MAX) {
            d.lds_tab = 1;
            need = edge_b + tab_b;
        } else if (tab_b) {
            d.tab_off = (int64_t)pl.ws_bytes;
            pl.ws_bytes += align256(tab_b);
        }
        if (need <= SLOT_MAX) {
            pl.slot_common = std::max(pl.slot_common, need);
            pl.pairs.push_back(d);
        } else {
            pl.slot_alone = std::max(pl.slot_alone, need);
            alone.push_back(d);
        }
    }
    pl.n_common = (int32_t)pl.pairs.size();
    pl.pairs.insert(pl.pairs.end(), alone.begin(), alone.end());
    pl.slot_common = (size_t)round_up((int64_t)pl.slot_common, 16);
    pl.slot_alone = (size_t)round_up((int64_t)pl.slot_alone, 8);
    return SCTC_OK;
}

template <bool OPS>
int launch_edit(const EditArgs& base, const EditPlan& pl, hipStream_t s)
{
    const int n_alone = (int)pl.pairs.size() - pl.n_common;
    if (pl.n_common) {
        EditArgs a = base;
        a.count = pl.n_common;
        a.slot = (int32_t)pl.slot_common;
        hipLaunchKernelGGL(edit_distance_kernel<OPS>, dim3((pl.n_common + WAVES - 1) / WAVES), dim3(64 * WAVES),
                           WAVES * pl.slot_common, s, a);
        SCTC_HIP_TRY(hipGetLastError());
    }
    if (n_alone) {      // a panel edge beyond 16 KB: one wave per workgroup, up to 8191 rows of 8 bytes
        EditArgs a = base;
        a.pairs = base.pairs + pl.n_common;
        a.count = n_alone;
        a.slot = (int32_t)pl.slot_alone;
        hipLaunchKernelGGL(edit_distance_kernel<OPS>, dim3(n_alone), dim3(64), pl.slot_alone, s, a);
        SCTC_HIP_TRY(hipGetLastError());
    }
    return SCTC_OK;
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_edit_distance_workspace_bytes(const sctc_edit_config* cfg, size_t* bytes)
{
    SCTC_CHECK_ARG(bytes, "edit: null bytes");
    *bytes = 0;
    EditPlan pl;
    SCTC_TRY(plan_edit(cfg, pl));
    *bytes = pl.ws_bytes;
    return SCTC_OK;
}

int sctc_edit_distance_batch(const sctc_edit_config* cfg, const int32_t* a_dev, const int32_t* b_dev,
                             int32_t* stats_dev, int8_t* ops_dev, int32_t* ops_len_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream)
{
    EditPlan pl;
    SCTC_TRY(plan_edit(cfg, pl));
    if (cfg->P == 0) return SCTC_OK;
    const bool want_ops = (cfg->flags & SCTC_EDIT_OPS) != 0;
    SCTC_CHECK_ARG(stats_dev, "edit: null stats");
    SCTC_CHECK_ARG((a_dev || !pl.any_a) && (b_dev || !pl.any_b), "edit: null sequences");
    if (want_ops) SCTC_CHECK_ARG(ops_len_dev && (ops_dev || pl.ops_total == 0), "edit: SCTC_EDIT_OPS without ops / ops_len");
    if (workspace_bytes < pl.ws_bytes || (pl.ws_bytes && !workspace_dev))
        return set_error(SCTC_ERR_WORKSPACE, "edit: workspace %zu bytes < %zu needed", workspace_dev ? workspace_bytes : (size_t)0,
                         pl.ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    // The descriptors stay in pinned host memory and every wave reads its own once: the counts mode needs no
    // workspace to upload them into.  A per-thread stage that lives as long as the process (capi_ctc.hip does the
    // same); its event keeps the buffer from being overwritten while a launch may still read it.
    static thread_local PinnedStage* stage = new PinnedStage();
    const size_t bytes = pl.pairs.size() * sizeof(EditPair);
    void* pin = stage->acquire(bytes);
    if (!pin) return set_error(SCTC_ERR_HIP, "edit: no pinned host memory for %zu bytes of pair descriptors", bytes);
    memcpy(pin, pl.pairs.data(), bytes);
    void* pin_dev = nullptr;
    SCTC_HIP_TRY(hipHostGetDevicePointer(&pin_dev, pin, 0));
    EditArgs a{};
    a.pairs = (const EditPair*)pin_dev;
    a.a = a_dev;
    a.b = b_dev;
    a.stats = stats_dev;
    a.ops = ops_dev;
    a.ops_len = ops_len_dev;
    a.ws = (char*)workspace_dev;
    PinnedUploadGuard guard(s, true);
    SCTC_TRY(want_ops ? launch_edit<true>(a, pl, s) : launch_edit<false>(a, pl, s));
    SCTC_HIP_TRY(stage->uploaded(s));
    guard.done();
    return SCTC_OK;
}

}  // extern "C"
