/*
 * sctc_diag.h -- C ABI of libsctc_diag.so: hardware probes used while developing and measuring
 * the kernels of libsctc_hip.so.  NOT part of the drop-in boundary (include/sctc.h): nothing in
 * stanford-ctc_amd/ loads this library; tests/gpu_diag.py, bench.py's "sustained peak" note and
 * __graft_entry__.smoke() do.  These entry points allocate (and free) their own scratch memory.
 * The library links against libsctc_hip.so for one purpose: the tests' doors below to the product's own GEMM
 * launcher (sctc_diag_gemm) and to its internal elementwise launchers.
 */
#ifndef SCTC_DIAG_H_
#define SCTC_DIAG_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* sctc_diag_last_error(void);
/* runs the cross-lane / MFMA fragment-layout probes the kernels rely on; 0 = all as expected,
 * else a bitmask of the failed probes */
int sctc_selftest(void* stream);
/* hand-off latencies between workgroups on the same / on different XCDs (flag ping-pong per
 * polling-load scope, 1 KiB tagged payload).  results_host[10]: partner block ids (same, cross
 * XCD), then microseconds per round trip: same-XCD {sc0, sc1, sc0+sc1}, cross-XCD {sc0, sc1,
 * sc0+sc1}, tagged payload {same, cross}; -1 = timed out (a scope that never observes the store) */
int sctc_probe_fabric(float* results_host, int32_t n_results, void* stream);
/* sustained fp32 matrix-pipe rate of register-only MFMA loops on every SIMD: results_host[8] =
 * {TFLOP/s, ms} for v_mfma_f32_32x32x2_f32 and v_mfma_f32_16x16x4_f32 with constant operands,
 * then the same two with fresh random operands per MFMA group */
int sctc_probe_mfma(float* results_host, int32_t n_results, void* stream);

/* flag-after-drain hand-off with IMMEDIATE plain loads by 15 consumer workgroups on other XCDs,
 * 20 000 fresh 1 KiB blocks.  results_host[9]: per mode {stale payload dwords, iterations (-1: timed
 * out), microseconds per iteration}; mode 0 = the recurrent kernels' protocol (drain, plain loads),
 * 1 = no drain (must show stale data), 2 = drain + L2-bypassing loads */
int sctc_probe_handoff(float* results_host, int32_t n_results, void* stream);
/* n_wgs workgroups of 256 threads that hold their compute units for `microseconds`: the stand-in
 * for a collective kernel on a side stream (one workgroup per channel, like RCCL) */
int sctc_diag_spin(void* stream, int32_t n_wgs, int32_t microseconds);

/* a stream whose kernels run only on the compute units whose bit is set in mask_words (n_words x 32
 * bits; hipExtStreamCreateWithCUMask) */
int sctc_diag_stream_cu_mask(const uint32_t* mask_words, int32_t n_words, void** stream_out);
int sctc_diag_stream_destroy(void* stream);
/* n_wgs workgroups of 256 threads, each holding its CU for hold_us: out_host[4 * i + {0,1,2,3}] =
 * XCC id, shader engine, shader array, CU id of workgroup i (synchronous) */
int sctc_diag_where(int32_t* out_host, int32_t n_wgs, int32_t hold_us, void* stream);

/* ---- test-only door to the product library's GEMM launcher (gemm_entry.hip; tests/test_gpu_gemm_options.py).
 * A plain-C mirror of sctc::GemmArgs (stanford-ctc_amd/csrc/gemm_f32.h), field for field and in its order;
 * sctc_diag_gemm copies it into a GemmArgs and calls sctc::launch_gemm_f32 OF libsctc_hip.so (this
 * library links against it: no second compilation of the kernels).  Errors: -1 / -2 with the message in the
 * PRODUCT library's sctc_last_error(). */
typedef struct sctc_diag_gemm_args {
    const void* A;          /* fp32, or 16-bit elements with in16 */
    const void* B;
    float* C;
    int64_t lda, ldb, ldc;
    int32_t M, N, K;
    int32_t a_kcontig, b_kcontig;
    const int32_t* idx_a;
    const int32_t* idx_b;
    const float* bias;
    const float* mask;
    int64_t ldmask;
    const float* addend;
    int64_t ldadd;
    float add_scale;
    int32_t relu;
    int32_t accumulate;
    float* colsum_a;
    float* splitk_ws;       /* splits * M * (N + 1) floats when splits > 1 */
    int32_t splits;
    int32_t prec;           /* 0 fp32, 1 float16, 2 bfloat16, 3 bf16x3 */
    int32_t in16;
    uint16_t* C16a;
    uint16_t* C16b;
    int64_t ldc16;
    int32_t skip_c32;
    const uint16_t* mask16;
    int64_t ldmask16;
    const float* A2;
    float* a_sum;
} sctc_diag_gemm_args;
int sctc_diag_gemm(const sctc_diag_gemm_args* args, void* stream);
/* sctc::gemm_plan (stanford-ctc_amd/csrc/gemm_plan.h) of these arguments under the process's current switches: what
 * sctc_diag_gemm would launch (no pointer is dereferenced, no GPU needed).  kernel: 0 fp32, 1 16-bit rounding in
 * registers, 2 16-bit operands staged through registers, 3 LDS-DMA, 4 bf16x3; splits / ws_floats: the split-K count
 * the product picks and the workspace floats it needs (0 when splits == 1). */
typedef struct sctc_diag_gemm_plan_out {
    int32_t kernel, bm, bn, bk, threads, occ, lds_bytes, grid_x, splits, split_tile_differs;
    int64_t ws_floats;
} sctc_diag_gemm_plan_out;
int sctc_diag_gemm_plan(const sctc_diag_gemm_args* args, sctc_diag_gemm_plan_out* out);
/* the same plan asked by shape alone (both operands row-contiguous, no gather): the split-K count through *splits, the
 * workspace floats it needs (0 when *splits == 1) returned */
int64_t sctc_diag_gemm_plan_splits(int32_t M, int32_t N, int32_t K, int32_t prec, int32_t in16, int32_t* splits);

/* ---- test-only door to the internal launchers of stanford-ctc_amd/csrc/elementwise.h (elementwise_entry.hip;
 * tests/test_gpu_elementwise.py): each entry passes its arguments to the sctc::launch_* function of libsctc_hip.so of
 * the same name and returns its code; the message of an error is in the PRODUCT library's sctc_last_error().
 * add / cvt16 / add16 move float4 groups: 16-byte aligned pointers, n a multiple of 4.  Nullable: both outputs of
 * cvt16, every output of add16, both shadows of gather_rows16. */
int sctc_diag_gather_rows(float* dst, int64_t ldd, const float* src, int64_t lds, const int32_t* idx, int64_t rows,
                          int32_t cols, void* stream);
int sctc_diag_scatter_rows(float* dst, int64_t ldd, const float* src, int64_t lds, const int32_t* idx, int64_t rows,
                           int32_t cols, void* stream);
int sctc_diag_add(float* out, const float* a, const float* b, int64_t n, void* stream);
int sctc_diag_cvt16(const float* src, uint16_t* dst_f16, uint16_t* dst_bf16, int64_t n, void* stream);
int sctc_diag_add16(float* out, const float* a, const float* b, uint16_t* o_f16, uint16_t* o_bf16, uint16_t* a_bf16,
                    uint16_t* b_bf16, int64_t n, void* stream);
int sctc_diag_transpose_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int32_t rows,
                             int32_t cols, void* stream);
int sctc_diag_gather_rows16(float* dst, uint16_t* d_f16, uint16_t* d_bf16, int64_t ldd, const float* src, int64_t lds,
                            const int32_t* idx, int64_t rows, int32_t cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif
