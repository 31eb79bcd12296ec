// The fixed-window feed-forward character LM on the device: the model as the
// kernels see it and the ONE routine that evaluates rows, log10 P(. | context) for a tile of up
// to 32 contexts.  The standalone rows kernel (nnlm.hip) and the prefix beam search
// (ctc_beam.hip, ctc_nnbeam_kernel) both call nnlm_tile and nothing else, so a row is the same
// function of its context wherever it is asked for.
//
//   layer 0      h_0 = relu(b_0 + sum over the K slots, oldest first, of column slot * V + id of W_0):
//                float32 additions in slot order, no product, no input matrix
//   layers 1..   out^T = W * in^T on v_mfma_f32_32x32x2_f32: the 32 contexts are the columns of the
//                accumulator tile (lane & 31), 32 units its rows; the four waves split the unit tiles.
//                The accumulator starts at the bias; k is consumed in the fixed order 0,4 1,5 2,6 3,7
//                8,12 ... (two k per instruction, one per half wave), an exact fma chain per output
//   rows         log10 softmax over the V outputs in float64, one wave per context
//
// Nothing in the chain of a context reads another context's data, the tile slot it sits in or
// the number of contexts in the tile: unused slots hold zeros and are never read back.
//
// Layouts (sctc_nnlm_create repacks):  W_0 column-major [K * V][H_1];  W_l, l >= 1, and the
// activations in quads of four consecutive k: X[k / 4][index][4], index = unit (weights, padded to a
// multiple of 32 with zero rows) or tile slot (activations), so that every operand load and every
// activation store is one float4 per lane, consecutive across the lanes.
#pragma once
#include "common.h"

namespace sctc {

constexpr int NN_TILE = 32;        // contexts per tile
constexpr int NN_THREADS = 256;    // the routine is written for four waves
constexpr int NN_MAX_LAYERS = 5;   // weight matrices: 1..4 hidden layers and the output layer
constexpr int NN_MAX_WIDTH = 2048;
constexpr int NN_MAX_CONTEXT = 32;
constexpr int NN_MAX_VOCAB = 256;

struct NNLMDev {
    const float* w[NN_MAX_LAYERS];
    const float* b[NN_MAX_LAYERS];
    int32_t width[NN_MAX_LAYERS + 1];   // width[0] = K * V, then the layer outputs as stored (padded)
    int32_t n_layers;
    int32_t V, Vp;                      // vocabulary, and padded to a multiple of 32
    int32_t K;                          // context slots
    int32_t bos, null_id;
    int32_t hmax;                       // widest hidden layer
};

// scratch of one tile: two activation buffers, the rows, the context ids
__host__ __device__ inline size_t nn_act_bytes(int hmax) { return align256((size_t)2 * NN_TILE * hmax * sizeof(float)); }
__host__ __device__ inline size_t nn_row_bytes(int Vp) { return align256((size_t)NN_TILE * Vp * sizeof(float)); }
__host__ __device__ inline size_t nn_ids_bytes(int K) { return align256((size_t)NN_TILE * K * sizeof(int32_t)); }
__host__ __device__ inline size_t nn_tile_bytes(int hmax, int Vp, int K)
{
    return nn_act_bytes(hmax) + nn_row_bytes(Vp) + nn_ids_bytes(K);
}

#ifdef __HIPCC__

typedef float nn_f32x16 __attribute__((ext_vector_type(16)));

// where a recurrent layer (REC, rnnlm_dev.h) leaves the new states: slot e < cnt to st + row[e] * Nout
struct NNStateOut {
    float* st;
    const int32_t* row;
    int cnt;
};

// one layer l >= 1 for the tile: TN unit tiles of 32 per wave and pass, all reading one activation
// operand.  LAST: the output layer, stored as plain rows z[slot][Vp] without the relu.  REC: the
// recurrent layer of rnnlm_dev.h -- the accumulator starts from the pre-activation of its own slot,
// which `out` holds in the quad layout (every lane reads exactly the quads it stores later, so the
// result replaces it in place), and the result is also stored as the state of the slot's entry.
template <int TN, bool LAST, bool REC = false>
__device__ __forceinline__ void nn_layer(const float* __restrict__ W, const float* __restrict__ bias,
                                         const float* __restrict__ in, float* __restrict__ out, int Hin, int Nout,
                                         NNStateOut so = NNStateOut{})
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int e = lane & 31, g = lane >> 5;
    const int nt = Nout >> 5, nj = Hin >> 3;
    for (int t0 = wv * TN; t0 < nt; t0 += 4 * TN) {
        nn_f32x16 acc[TN];
        const float4* wp[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int tile = min(t0 + i, nt - 1);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 bv;
                if constexpr (REC) bv = reinterpret_cast<const float4*>(out)[(size_t)(tile * 8 + rq * 2 + g) * NN_TILE + e];
                else bv = reinterpret_cast<const float4*>(bias)[tile * 8 + rq * 2 + g];
                acc[i][4 * rq + 0] = bv.x;
                acc[i][4 * rq + 1] = bv.y;
                acc[i][4 * rq + 2] = bv.z;
                acc[i][4 * rq + 3] = bv.w;
            }
            wp[i] = reinterpret_cast<const float4*>(W) + (size_t)g * Nout + tile * 32 + e;
        }
        const float4* ip = reinterpret_cast<const float4*>(in) + g * NN_TILE + e;
        // quad 2j + g of the k axis: k = 8j + 4g .. + 3
        float4 bq = ip[0], aq[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) aq[i] = wp[i][0];
        for (int j = 0; j < nj; ++j) {
            float4 bn = bq, an[TN];
#pragma unroll
            for (int i = 0; i < TN; ++i) an[i] = aq[i];
            if (j + 1 < nj) {
                bn = ip[(size_t)(2 * j + 2) * NN_TILE];
#pragma unroll
                for (int i = 0; i < TN; ++i) an[i] = wp[i][(size_t)(2 * j + 2) * Nout];
            }
#pragma unroll
            for (int i = 0; i < TN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[i].x, bq.x, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[i].y, bq.y, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[i].z, bq.z, acc[i], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[i].w, bq.w, acc[i], 0, 0, 0);
            bq = bn;
#pragma unroll
            for (int i = 0; i < TN; ++i) aq[i] = an[i];
        }
        // lane (slot e, half g), register r: unit tile * 32 + 8 (r / 4) + 4 g + r % 4
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int tile = t0 + i;
            if (tile >= nt) continue;
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float4 v = make_float4(acc[i][4 * rq], acc[i][4 * rq + 1], acc[i][4 * rq + 2], acc[i][4 * rq + 3]);
                if constexpr (LAST) {
                    *reinterpret_cast<float4*>(out + (size_t)e * Nout + tile * 32 + rq * 8 + g * 4) = v;
                } else {
                    v.x = fmaxf(v.x, 0.0f);
                    v.y = fmaxf(v.y, 0.0f);
                    v.z = fmaxf(v.z, 0.0f);
                    v.w = fmaxf(v.w, 0.0f);
                    reinterpret_cast<float4*>(out)[(size_t)(tile * 8 + rq * 2 + g) * NN_TILE + e] = v;
                    if constexpr (REC) {
                        if (e < so.cnt)
                            *reinterpret_cast<float4*>(so.st + (size_t)so.row[e] * Nout + tile * 32 + rq * 8 + g * 4) = v;
                    }
                }
            }
        }
    }
}

// rows[slot * Vp + v], v < V, of `cnt` slots: the outputs z on entry, log10 softmax(z) on return, in
// float64, one wave per slot; V <= 256 = 4 values per lane
__device__ __forceinline__ void nn_log10_softmax(float* rows, int cnt, int V, int Vp)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int e = wv; e < cnt; e += 4) {
        double z[4], mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = lane + 64 * i;
            z[i] = v < V ? (double)rows[(size_t)e * Vp + v] : -INFINITY;
            mx = fmax(mx, z[i]);
        }
        for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (lane + 64 * i < V) s += exp(z[i] - mx);
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        const double lse = mx + log(s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = lane + 64 * i;
            if (v < V) rows[(size_t)e * Vp + v] = (float)((z[i] - lse) * 0.43429448190325182765);
        }
    }
}

// Rows of `cnt` (1..32) contexts: ids[slot * K + s] are the LM ids of the window, oldest first, each
// in 0..V-1.  On return rows[slot * Vp + v], v < V, holds log10 P(v | context of slot).  `act` is
// nn_act_bytes(hmax) of scratch.  Every thread of the 256-thread workgroup calls it with the same
// arguments; whatever the caller wrote to `ids` must be ordered by a barrier before the call, and
// the routine ends with one.
__device__ __forceinline__ void nnlm_tile(const NNLMDev& m, const int32_t* ids, int cnt,
                                          float* act, float* rows)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int H1 = m.width[1], K = m.K, V = m.V;
    float* bufs[2] = {act, act + (size_t)NN_TILE * m.hmax};

    // ---- layer 0: K columns and the bias, one wave per context, the lanes along the units ----
    for (int e = wv; e < NN_TILE; e += 4) {
        for (int q = lane; q < (H1 >> 2); q += 64) {
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (e < cnt) {
                acc = reinterpret_cast<const float4*>(m.b[0])[q];
                for (int s = 0; s < K; ++s) {
                    const int col = s * V + ids[e * K + s];
                    const float4 c4 = reinterpret_cast<const float4*>(m.w[0] + (size_t)col * H1)[q];
                    acc.x += c4.x;
                    acc.y += c4.y;
                    acc.z += c4.z;
                    acc.w += c4.w;
                }
                acc.x = fmaxf(acc.x, 0.0f);
                acc.y = fmaxf(acc.y, 0.0f);
                acc.z = fmaxf(acc.z, 0.0f);
                acc.w = fmaxf(acc.w, 0.0f);
            }
            reinterpret_cast<float4*>(bufs[0])[(size_t)q * NN_TILE + e] = acc;
        }
    }
    __syncthreads();

    // ---- layers 1 .. L on the matrix cores ----
    int cur = 0;
    for (int l = 1; l < m.n_layers; ++l) {
        const int Hin = m.width[l], Nout = m.width[l + 1];
        const bool last = l == m.n_layers - 1;
        if (last) {
            nn_layer<1, true>(m.w[l], m.b[l], bufs[cur], rows, Hin, Nout);
        } else if (Nout >= 512) {
            nn_layer<4, false>(m.w[l], m.b[l], bufs[cur], bufs[cur ^ 1], Hin, Nout);
        } else {
            nn_layer<1, false>(m.w[l], m.b[l], bufs[cur], bufs[cur ^ 1], Hin, Nout);
        }
        cur ^= 1;
        __syncthreads();
    }

    nn_log10_softmax(rows, cnt, V, m.Vp);
    __syncthreads();
}

#endif  // __HIPCC__

}  // namespace sctc

// the handle of include/sctc.h
struct sctc_nnlm {
    sctc::NNLMDev dev;
    char* mem = nullptr;            // one allocation: parameters, then the scratch of the rows kernel
    char* scratch = nullptr;        // rows_blocks tiles
    size_t bytes = 0;
    int32_t rows_blocks = 0;
    int device = -1;
};
