// The recurrent character LM on the device: the model as the kernels see it and
// the ONE routine that makes a recurrent step, for a tile of up to 32 (parent state, LM id) pairs:
//
//   h' = relu(bh + Wx[:, id] + Wh h)        row = log10 softmax(Wo h' + bo)
//
// The step kernel (rnnlm.hip) and the prefix beam search (ctc_beam.hip, ctc_rnnbeam_kernel) both
// call rnnlm_tile and nothing else, so a state and a row are the same function of the prefix
// wherever they are asked for.
//
//   pre-activation   bh + column id of Wx: one float32 addition per unit, no product
//   recurrent layer  nn_layer of nnlm_dev.h in its REC mode: the same operand maps, k order and
//                    lookahead; the accumulator of a slot starts from its own pre-activation, the
//                    activation operand is the 32 parent states gathered into the quad layout
//   output layer     nn_layer<1, true>, then nn_log10_softmax: the code the window model runs
//
// Nothing in the chain of a slot reads another slot, the slot's position or the number of slots in
// the tile.  A zero parent state (the empty prefix) goes the same way: every fma of its chain adds
// a zero product, which leaves the accumulator as it is.
//
// Layouts (sctc_rnnlm_create repacks):  Wx column-major [V][H];  Wh and Wo in quads of four
// consecutive k, X[k / 4][unit][4], Wo with zero rows up to Vp;  states row-major [entry][H].
#pragma once
#include "nnlm_dev.h"

namespace sctc {

struct RNNLMDev {
    const float* wx;   // [V][H]
    const float* wh;   // [H / 4][H][4]
    const float* bh;   // [H]
    const float* wo;   // [H / 4][Vp][4]
    const float* bo;   // [Vp]
    int32_t V, Vp;     // vocabulary, and padded to a multiple of 32
    int32_t H;         // hidden units, a multiple of 32
    int32_t bos;
};

// scratch of one tile: pre-activation / new state and the gathered parent states (nn_act_bytes), the
// rows, and three ints per slot (LM id, parent's state row, the entry's state row)
constexpr int RNN_SLOT_INTS = 3 * NN_TILE;
__host__ __device__ inline size_t rnn_tile_bytes(int H, int Vp)
{
    return nn_act_bytes(H) + nn_row_bytes(Vp) + align256(RNN_SLOT_INTS * sizeof(int32_t));
}

#ifdef __HIPCC__

// One recurrent step of `cnt` (1..32) slots.  slot[e] is the LM id fed (0..V-1), slot[32 + e] the row
// of the parent's state in `sin` ([.][H]; nullptr: every parent state is zero) and slot[64 + e] the
// row of `sout` that receives the new state.  Unless `rows` is nullptr, rows[e * Vp + v], v < V, holds
// log10 P(v | the prefix the new state stands for) on return.  `act` is nn_act_bytes(H) of scratch.
// Every thread of the 256-thread workgroup calls it with the same arguments; what the caller wrote to
// `slot` must be ordered by a barrier before the call, and the routine ends with one.  sin and sout
// may not overlap in the rows the tile reads and writes, unless slot e writes the row it reads.
__device__ __forceinline__ void rnnlm_tile(const RNNLMDev& m, const int32_t* slot, int cnt, const float* sin,
                                           float* sout, float* act, float* rows)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int H = m.H;
    float* pre = act;                              // X[k / 4][slot][4]: bh + Wx[:, id], then h'
    float* par = act + (size_t)NN_TILE * H;        // the parent states in the same layout

    // ---- pre-activation and the gather, one wave per slot, the lanes along the units ----
    for (int e = wv; e < NN_TILE; e += 4) {
        for (int q = lane; q < (H >> 2); q += 64) {
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hp = acc;
            if (e < cnt) {
                acc = reinterpret_cast<const float4*>(m.bh)[q];
                const float4 c4 = reinterpret_cast<const float4*>(m.wx + (size_t)slot[e] * H)[q];
                acc.x += c4.x;
                acc.y += c4.y;
                acc.z += c4.z;
                acc.w += c4.w;
                if (sin) hp = reinterpret_cast<const float4*>(sin + (size_t)slot[NN_TILE + e] * H)[q];
            }
            reinterpret_cast<float4*>(pre)[(size_t)q * NN_TILE + e] = acc;
            reinterpret_cast<float4*>(par)[(size_t)q * NN_TILE + e] = hp;
        }
    }
    __syncthreads();

    // ---- the recurrent layer on the matrix cores: pre <- relu(pre + Wh par), and the new states ----
    const NNStateOut so{sout, slot + 2 * NN_TILE, cnt};
    if (H >= 512) nn_layer<4, false, true>(m.wh, nullptr, par, pre, H, H, so);
    else nn_layer<1, false, true>(m.wh, nullptr, par, pre, H, H, so);
    __syncthreads();

    if (rows) {
        nn_layer<1, true>(m.wo, m.bo, pre, rows, H, m.Vp);
        __syncthreads();
        nn_log10_softmax(rows, cnt, m.V, m.Vp);
        __syncthreads();
    }
}

#endif  // __HIPCC__

}  // namespace sctc

// the handle of include/sctc.h
struct sctc_rnnlm {
    sctc::RNNLMDev dev;
    char* mem = nullptr;        // one allocation: parameters, then the scratch of sctc_rnnlm_step
    char* scratch = nullptr;    // step_blocks tiles
    size_t bytes = 0;
    int32_t step_blocks = 0;
    int device = -1;
};
