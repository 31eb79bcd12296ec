// Persistent weight-stationary kernel for the bi-directional recurrence
// (brnnet.py:143-153 forward, :206-224 backprop through time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recurrent_plan.h"

namespace sctc {

// Two independent recurrences ("groups") run in one launch on disjoint CUs:
//   forward pass : group 0 = hFor (time ascending, Wf), group 1 = hBack (descending, Wb)
//   BPTT         : group 0 = deltasFor (descending, Wf^T, mask from hFor),
//                  group 1 = deltasBack (ascending, Wb^T, mask from hBack)
// Rows follow the packed time-major minibatch layout: frame t of utterance b
// (utterances sorted by length, longest first) is row rowbase[t] + b.
struct RecArgs {
    const float* W[2];      // [Hp][ldw] row-major recurrent weight of each group
    int64_t ldw;
    int32_t transpose;      // 0: out = W x (forward); 1: out = W^T x (BPTT)
    int32_t descending[2];  // time order of each group
    const float* pre[2];    // [rows][ld]: z (forward) / deltasOut (BPTT): the term added per frame
    const float* act[2];    // BPTT only: stored hFor/hBack for the (0,maxAct) mask; else NULL
    float* out[2];          // [rows][ld]
    int64_t ld;
    int32_t Hp;             // padded layer size (multiple of 32)
    int32_t B;              // utterances
    int32_t Tmax;
    const int32_t* rowbase; // device [Tmax]
    const int32_t* T_b;     // device [B] (sorted, descending)
    float max_act;          // <= 0: no ceiling
    // Exchange buffer: chunk-major copy of the state, [2 groups][Hp/16][n_xrows][16] floats.
    // Exchange row of utterance b at STEP j = xbase[j] + b; xbase rounds every step's
    // block up to 4 rows (256 B) so that no cache line holds data of two different steps,
    // and up to 16 rows from 17 alive utterances on (recurrent_step_xrows below).
    float* xbuf;
    const int32_t* xbase;   // device [Tmax]
    int32_t n_xrows;
    unsigned* counters;     // [REC_COUNTER_WORDS]: sticky error word at [2], per-producer step flags from [32]
    int32_t sync_mode;      // 0: plain exchange stores + agent-scope release fence before the flag
                            // 1: write-through (sc1) exchange stores, no fence
    int32_t poll_delay;     // s_sleep units (64 cycles) before the first poll of a step; < 0: pick by layer size
    int32_t variant;        // a RecVariant (recurrent_plan.h): kernel selection overrides, A/Bs, diagnostics
    unsigned* debug;        // nullable: s_memtime stamps [2 wgs][16 steps][8] for steps 64..79
    int32_t b_off;          // rank of this launch's first utterance in the packed minibatch (minibatches of
                            // more than 128 utterances run as several launches; T_b already points at it)
    const int32_t* T_host;  // nullable: host copy of the full (sorted) T_b, used to shorten later launches
    int32_t linear_map;     // two-chain kernel: linear block -> (chain, producer) map, chain = direction (the single-chain launch of
                            // 4..16 utterances; set by the launcher -- `variant` keeps its A/B meaning, e.g. REC_V_ROW_MAJOR, there too)
    int32_t prec16;         // != 0: "fp16 activations" -- the 6..16-utterance kernel exchanges the state
                            // and holds the weights in 16 bit (float16 forward, bfloat16 BPTT), fp32 accumulate
};
// [2 wgs][16 steps][8] s_memtime stamps of steps 64..79, then [512 workgroups][8] wall-clock
// (100 MHz, global) stamps of step 70 for every workgroup
static constexpr int REC_DEBUG_ALL_OFF = 2 * 16 * 8;
static constexpr int REC_DEBUG_WORDS = 2 * 16 * 8 + 512 * 8;
#ifndef SCTC_REC_FLAG_STRIDE
#define SCTC_REC_FLAG_STRIDE 8
#endif
// words between the step flags of two producers (32 = one 128-byte line per flag)
static constexpr int REC_FLAG_STRIDE = SCTC_REC_FLAG_STRIDE;
static constexpr int REC_COUNTER_WORDS = 32 + 4 * 128 * REC_FLAG_STRIDE;   // error word + up to 4 chains x 128 producers

// Exchange rows of a time step whose `alive` utterances are still running: a multiple of 4 (256 bytes: no cache line
// holds data of two steps); from 17 utterances on a multiple of 16, so that every tile of 16 utterances that is alive at
// all has its 16 rows inside the step's block and keeps the lane-order layout (recurrent.hip, lane_order_steps).
static inline int recurrent_step_xrows(int alive) { return alive >= 17 ? (alive + 15) & ~15 : (alive + 3) & ~3; }
// exchange rows needed for `rows` frames spread over `tmax` time steps (worst case: 3 rows of padding per step, 12 more
// for each of the at most rows / 17 steps with 17 or more utterances alive)
static inline int64_t recurrent_xrows_bound(int64_t rows, int64_t tmax) { return rows + 3 * tmax + 12 * (rows / 17 + 1); }
size_t recurrent_xbuf_floats(int Hp, int64_t max_xrows);
int recurrent_supported(int Hp, int B, char* why, int why_len);
// which path a launch_recurrent call took (`path` out-parameter, nullable)
static constexpr int REC_PATH_NONE = 0;
static constexpr int REC_PATH_PERSISTENT = 1;          // one whole-device persistent launch per pass
static constexpr int REC_PATH_PERSISTENT_LEASED = 2;   // the same under the inter-process device lease
static constexpr int REC_PATH_FALLBACK = 3;            // one launch per time step (no spinning)
// Work of the caller's that runs on ANOTHER stream beside a persistent grid (REC_V_T_HALF / REC_V_T_CLAIM: a grid that
// leaves a GEMM block no LDS on its CUs).  fn(ctx) is called at most once, directly in front of the grid's launch -- the step
// flags are zero on `stream` by then -- and only for such a grid launched through the in-process gate: not under the device
// lease, not on the per-step fallback, not for a minibatch cut into several launches (`called` stays 0).  It forks the other
// stream off `stream` and holds it (hipStreamWaitValue32) until rec_resident_word(counters, g), g = 0, 1, are >= 2.
struct RecBeside {
    int (*fn)(void* ctx);
    void* ctx;
    int called;
};
// The tiled kernel's step flag of chain (direction g, sub-chain A), producer 0: j + 1 once its step j is published.  Step 1 is
// computed from the step-0 results of EVERY producer of the chain, and every workgroup of direction g is one: the word reaches
// 2 (the minibatch's longest utterance has >= 2 frames) only after all workgroups of that direction have become resident.
static inline unsigned* rec_resident_word(unsigned* counters, int g) { return counters + 32 + (size_t)(g * 2 * 64) * REC_FLAG_STRIDE; }
int launch_recurrent(const RecArgs& a, hipStream_t stream, int* path = nullptr, RecBeside* beside = nullptr);
// clears the sticky error word (counters[2]): once per step, before its first recurrent launch
int recurrent_clear_error(unsigned* counters, hipStream_t stream);
// shared-device mode: persistent launches take an inter-process lease (flock on a per-device file)
// and run synchronously.  Initial value: SCTC_SHARED_DEVICE in the environment.  The state and the guards
// it switches are host code of their own: device_share.h (SharedMode).
int recurrent_shared_device_mode();
void recurrent_set_shared_device_mode(int on);

}  // namespace sctc
