// The recurrent character LM of the prefix beam search: the handle (parameters
// repacked for rnnlm_dev.h and uploaded once), and one recurrent step for arbitrary (state, id)
// pairs -- the same rnnlm_tile the search calls, one tile of 32 pairs per workgroup and pass.
#include <vector>

#include "common.h"
#include "rnnlm_dev.h"

namespace sctc {
namespace {

constexpr int STEP_BLOCKS = 64;    // tiles in flight in sctc_rnnlm_step: their scratch lives in the handle

struct StepArgs {
    RNNLMDev m;
    const int32_t* ids;      // [n]
    const float* state_in;   // [n][H] or nullptr
    float* state_out;        // [n][H]
    float* rows;             // [n][V] or nullptr
    char* scratch;           // gridDim.x tiles
    int64_t n;
};

__global__ __launch_bounds__(NN_THREADS) void rnnlm_step_kernel(StepArgs p)
{
    const RNNLMDev& m = p.m;
    const int V = m.V, Vp = m.Vp, H = m.H;
    char* w = p.scratch + (size_t)blockIdx.x * rnn_tile_bytes(H, Vp);
    float* act = (float*)w;
    float* rows = (float*)(w + nn_act_bytes(H));
    int32_t* slot = (int32_t*)(w + nn_act_bytes(H) + nn_row_bytes(Vp));
    const int64_t tiles = (p.n + NN_TILE - 1) / NN_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * NN_TILE;
        const int cnt = (int)min((int64_t)NN_TILE, p.n - first);
        // an id outside the vocabulary would index outside Wx: clamped.  Pair e of the tile reads and
        // writes row e of the tile's part of the state arrays.
        if (threadIdx.x < cnt) {
            slot[threadIdx.x] = min(max(p.ids[first + threadIdx.x], 0), V - 1);
            slot[NN_TILE + threadIdx.x] = threadIdx.x;
            slot[2 * NN_TILE + threadIdx.x] = threadIdx.x;
        }
        __syncthreads();
        rnnlm_tile(m, slot, cnt, p.state_in ? p.state_in + first * H : nullptr, p.state_out + first * H, act,
                   p.rows ? rows : nullptr);
        if (p.rows)
            for (int i = threadIdx.x; i < cnt * V; i += NN_THREADS) {
                const int e = i / V, v = i - e * V;
                p.rows[first * V + i] = rows[(size_t)e * Vp + v];
            }
        __syncthreads();
    }
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_rnnlm_create(int32_t vocab, int32_t hidden, const float* wx_host, const float* wh_host,
                      const float* bh_host, const float* wo_host, const float* bo_host, int32_t bos_id,
                      sctc_rnnlm_t* out)
{
    SCTC_CHECK_ARG(out, "rnnlm: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(wx_host && wh_host && bh_host && wo_host && bo_host, "rnnlm: null parameters");
    SCTC_CHECK_ARG(vocab >= 3 && vocab <= NN_MAX_VOCAB, "rnnlm: vocabulary %d outside 3..%d", vocab, NN_MAX_VOCAB);
    SCTC_CHECK_ARG(hidden >= 32 && hidden <= NN_MAX_WIDTH && hidden % 32 == 0,
                   "rnnlm: hidden width %d is not a multiple of 32 in 32..%d", hidden, NN_MAX_WIDTH);
    SCTC_CHECK_ARG(bos_id >= 0 && bos_id < vocab, "rnnlm: <s> id %d outside the vocabulary", bos_id);
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));

    const int V = vocab, H = hidden, Vp = (int)round_up(vocab, 32);
    const size_t sz[5] = {align256((size_t)V * H * sizeof(float)), align256((size_t)H * H * sizeof(float)),
                          align256((size_t)H * sizeof(float)), align256((size_t)H * Vp * sizeof(float)),
                          align256((size_t)Vp * sizeof(float))};
    size_t off[5], total = 0;
    for (int i = 0; i < 5; ++i) {
        off[i] = total;
        total += sz[i];
    }
    const size_t param_bytes = total;
    total += (size_t)STEP_BLOCKS * rnn_tile_bytes(H, Vp);

    // repack on the host (rnnlm_dev.h): Wx by columns, Wh and Wo in quads of k, Wo with zero rows up to Vp
    std::vector<float> host(param_bytes / sizeof(float), 0.0f);
    float* d = host.data() + off[0] / sizeof(float);
    for (int n = 0; n < H; ++n)
        for (int c = 0; c < V; ++c) d[(size_t)c * H + n] = wx_host[(size_t)n * V + c];
    d = host.data() + off[1] / sizeof(float);
    for (int n = 0; n < H; ++n)
        for (int k = 0; k < H; ++k) d[((size_t)(k >> 2) * H + n) * 4 + (k & 3)] = wh_host[(size_t)n * H + k];
    memcpy(host.data() + off[2] / sizeof(float), bh_host, (size_t)H * sizeof(float));
    d = host.data() + off[3] / sizeof(float);
    for (int n = 0; n < V; ++n)
        for (int k = 0; k < H; ++k) d[((size_t)(k >> 2) * Vp + n) * 4 + (k & 3)] = wo_host[(size_t)n * H + k];
    memcpy(host.data() + off[4] / sizeof(float), bo_host, (size_t)V * sizeof(float));

    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, total);
    if (e == hipSuccess) e = hipMemcpy(mem, host.data(), param_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        return set_error(SCTC_ERR_HIP, "rnnlm: upload failed: %s", hipGetErrorString(e));
    }
    sctc_rnnlm* lm = new sctc_rnnlm();
    lm->mem = (char*)mem;
    lm->scratch = lm->mem + param_bytes;
    lm->bytes = total;
    lm->step_blocks = STEP_BLOCKS;
    lm->device = dev;
    RNNLMDev& m = lm->dev;
    m.wx = (const float*)(lm->mem + off[0]);
    m.wh = (const float*)(lm->mem + off[1]);
    m.bh = (const float*)(lm->mem + off[2]);
    m.wo = (const float*)(lm->mem + off[3]);
    m.bo = (const float*)(lm->mem + off[4]);
    m.V = V;
    m.Vp = Vp;
    m.H = H;
    m.bos = bos_id;
    *out = lm;
    return SCTC_OK;
}

int sctc_rnnlm_destroy(sctc_rnnlm_t lm)
{
    if (!lm) return SCTC_OK;
    if (lm->mem) (void)hipFree(lm->mem);
    delete lm;
    return SCTC_OK;
}

size_t sctc_rnnlm_bytes(sctc_rnnlm_t lm) { return lm ? lm->bytes : 0; }

int sctc_rnnlm_step(sctc_rnnlm_t lm, const int32_t* ids_dev, const float* state_in_dev, int64_t n,
                    float* state_out_dev, float* rows_dev, void* stream)
{
    SCTC_CHECK_ARG(lm, "rnnlm_step: null LM");
    SCTC_CHECK_ARG(n >= 0, "rnnlm_step: %lld pairs", (long long)n);
    if (n == 0) return SCTC_OK;
    SCTC_CHECK_ARG(ids_dev && state_out_dev, "rnnlm_step: null device pointer");
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    SCTC_CHECK_ARG(dev == lm->device, "rnnlm_step: the LM lives on device %d, the current device is %d", lm->device, dev);
    StepArgs a{};
    a.m = lm->dev;
    a.ids = ids_dev;
    a.state_in = state_in_dev;
    a.state_out = state_out_dev;
    a.rows = rows_dev;
    a.scratch = lm->scratch;
    a.n = n;
    const int64_t tiles = (n + NN_TILE - 1) / NN_TILE;
    const int grid = (int)(tiles < lm->step_blocks ? tiles : lm->step_blocks);
    hipLaunchKernelGGL(rnnlm_step_kernel, dim3(grid), dim3(NN_THREADS), 0, (hipStream_t)stream, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
