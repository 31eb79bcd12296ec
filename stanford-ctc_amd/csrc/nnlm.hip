// The neural character LM of the prefix beam search: the handle (parameters
// repacked for nnlm_dev.h and uploaded once), and rows for arbitrary contexts -- the same
// nnlm_tile the search calls, one tile of 32 contexts per workgroup and pass.
#include <vector>

#include "common.h"
#include "nnlm_dev.h"

namespace sctc {
namespace {

constexpr int ROWS_BLOCKS = 64;    // tiles in flight in sctc_nnlm_rows: their scratch lives in the handle

struct RowsArgs {
    NNLMDev m;
    const int32_t* ctx;   // [n * K]
    float* out;           // [n * V]
    char* scratch;        // gridDim.x tiles
    int64_t n;
};

__global__ __launch_bounds__(NN_THREADS) void nnlm_rows_kernel(RowsArgs p)
{
    const NNLMDev& m = p.m;
    const int K = m.K, V = m.V, Vp = m.Vp;
    char* w = p.scratch + (size_t)blockIdx.x * nn_tile_bytes(m.hmax, Vp, K);
    float* act = (float*)w;
    float* rows = (float*)(w + nn_act_bytes(m.hmax));
    int32_t* ids = (int32_t*)(w + nn_act_bytes(m.hmax) + nn_row_bytes(Vp));
    const int64_t tiles = (p.n + NN_TILE - 1) / NN_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * NN_TILE;
        const int cnt = (int)min((int64_t)NN_TILE, p.n - first);
        // an id outside the vocabulary would index outside the first weight matrix: clamped
        for (int i = threadIdx.x; i < cnt * K; i += NN_THREADS) ids[i] = min(max(p.ctx[first * K + i], 0), V - 1);
        __syncthreads();
        nnlm_tile(m, ids, cnt, act, rows);
        for (int i = threadIdx.x; i < cnt * V; i += NN_THREADS) {
            const int e = i / V, v = i - e * V;
            p.out[first * V + i] = rows[(size_t)e * Vp + v];
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_nnlm_create(int32_t vocab, int32_t context, int32_t n_layers, const int32_t* widths,
                     const float* const* weights_host, const float* const* biases_host, int32_t bos_id,
                     int32_t null_id, sctc_nnlm_t* out)
{
    SCTC_CHECK_ARG(out, "nnlm: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(widths && weights_host && biases_host, "nnlm: null argument");
    SCTC_CHECK_ARG(vocab >= 3 && vocab <= NN_MAX_VOCAB, "nnlm: vocabulary %d outside 3..%d", vocab, NN_MAX_VOCAB);
    SCTC_CHECK_ARG(context >= 1 && context <= NN_MAX_CONTEXT, "nnlm: context %d outside 1..%d", context,
                   NN_MAX_CONTEXT);
    SCTC_CHECK_ARG(n_layers >= 2 && n_layers <= NN_MAX_LAYERS, "nnlm: %d weight matrices outside 2..%d", n_layers,
                   NN_MAX_LAYERS);
    SCTC_CHECK_ARG(widths[0] == vocab * context, "nnlm: input width %d is not context * vocabulary = %d", widths[0],
                   vocab * context);
    SCTC_CHECK_ARG(widths[n_layers] == vocab, "nnlm: output width %d is not the vocabulary %d", widths[n_layers],
                   vocab);
    for (int l = 1; l < n_layers; ++l)
        SCTC_CHECK_ARG(widths[l] >= 32 && widths[l] <= NN_MAX_WIDTH && widths[l] % 32 == 0,
                       "nnlm: hidden width %d (layer %d) is not a multiple of 32 in 32..%d", widths[l], l,
                       NN_MAX_WIDTH);
    for (int l = 0; l < n_layers; ++l)
        SCTC_CHECK_ARG(weights_host[l] && biases_host[l], "nnlm: null parameters of layer %d", l);
    SCTC_CHECK_ARG(bos_id >= 0 && bos_id < vocab && null_id >= 0 && null_id < vocab && bos_id != null_id,
                   "nnlm: <s> id %d / <null> id %d outside the vocabulary or equal", bos_id, null_id);
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));

    const int Vp = (int)round_up(vocab, 32);
    int stored[NN_MAX_LAYERS + 1];
    for (int l = 0; l <= n_layers; ++l) stored[l] = widths[l];
    stored[n_layers] = Vp;
    int hmax = 0;
    for (int l = 1; l < n_layers; ++l) hmax = hmax > widths[l] ? hmax : widths[l];
    size_t woff[NN_MAX_LAYERS], boff[NN_MAX_LAYERS], total = 0;
    for (int l = 0; l < n_layers; ++l) {
        woff[l] = total;
        total += align256((size_t)stored[l] * stored[l + 1] * sizeof(float));
        boff[l] = total;
        total += align256((size_t)stored[l + 1] * sizeof(float));
    }
    const size_t param_bytes = total;
    const size_t tile = nn_tile_bytes(hmax, Vp, context);
    total += (size_t)ROWS_BLOCKS * tile;

    // repack on the host (nnlm_dev.h): W_0 by columns, the others in quads of k with zero rows up to Vp
    std::vector<float> host(param_bytes / sizeof(float), 0.0f);
    {
        const int KV = widths[0], H1 = widths[1];
        float* d = host.data() + woff[0] / sizeof(float);
        for (int n = 0; n < H1; ++n)
            for (int c = 0; c < KV; ++c) d[(size_t)c * H1 + n] = weights_host[0][(size_t)n * KV + c];
        memcpy(host.data() + boff[0] / sizeof(float), biases_host[0], (size_t)H1 * sizeof(float));
    }
    for (int l = 1; l < n_layers; ++l) {
        const int Hin = widths[l], Nout = widths[l + 1], Np = stored[l + 1];
        float* d = host.data() + woff[l] / sizeof(float);
        for (int n = 0; n < Nout; ++n)
            for (int k = 0; k < Hin; ++k)
                d[((size_t)(k >> 2) * Np + n) * 4 + (k & 3)] = weights_host[l][(size_t)n * Hin + k];
        memcpy(host.data() + boff[l] / sizeof(float), biases_host[l], (size_t)Nout * sizeof(float));
    }

    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, total);
    if (e == hipSuccess) e = hipMemcpy(mem, host.data(), param_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        return set_error(SCTC_ERR_HIP, "nnlm: upload failed: %s", hipGetErrorString(e));
    }
    sctc_nnlm* lm = new sctc_nnlm();
    lm->mem = (char*)mem;
    lm->scratch = lm->mem + param_bytes;
    lm->bytes = total;
    lm->rows_blocks = ROWS_BLOCKS;
    lm->device = dev;
    NNLMDev& m = lm->dev;
    memset(&m, 0, sizeof(m));
    for (int l = 0; l < n_layers; ++l) {
        m.w[l] = (const float*)(lm->mem + woff[l]);
        m.b[l] = (const float*)(lm->mem + boff[l]);
    }
    for (int l = 0; l <= n_layers; ++l) m.width[l] = stored[l];
    m.n_layers = n_layers;
    m.V = vocab;
    m.Vp = Vp;
    m.K = context;
    m.bos = bos_id;
    m.null_id = null_id;
    m.hmax = hmax;
    *out = lm;
    return SCTC_OK;
}

int sctc_nnlm_destroy(sctc_nnlm_t lm)
{
    if (!lm) return SCTC_OK;
    if (lm->mem) (void)hipFree(lm->mem);
    delete lm;
    return SCTC_OK;
}

size_t sctc_nnlm_bytes(sctc_nnlm_t lm) { return lm ? lm->bytes : 0; }

int sctc_nnlm_rows(sctc_nnlm_t lm, const int32_t* contexts_dev, int64_t n, float* rows_dev, void* stream)
{
    SCTC_CHECK_ARG(lm, "nnlm_rows: null LM");
    SCTC_CHECK_ARG(n >= 0, "nnlm_rows: %lld contexts", (long long)n);
    if (n == 0) return SCTC_OK;
    SCTC_CHECK_ARG(contexts_dev && rows_dev, "nnlm_rows: null device pointer");
    RowsArgs a{};
    a.m = lm->dev;
    a.ctx = contexts_dev;
    a.out = rows_dev;
    a.scratch = lm->scratch;
    a.n = n;
    const int64_t tiles = (n + NN_TILE - 1) / NN_TILE;
    const int grid = (int)(tiles < lm->rows_blocks ? tiles : lm->rows_blocks);
    hipLaunchKernelGGL(nnlm_rows_kernel, dim3(grid), dim3(NN_THREADS), 0, (hipStream_t)stream, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // extern "C"
