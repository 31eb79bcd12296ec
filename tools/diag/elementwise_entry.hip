// Test-only door to the internal launchers of stanford-ctc_amd/csrc/elementwise.hip (row gather / scatter, the
// float4 sum, the 16-bit shadow producers, the bfloat16 transpose): the public ABI reaches them only through a whole
// sctc_brnn_cost_and_grad.  Thin pass-throughs to the sctc::launch_* symbols of libsctc_hip.so, which this library
// LINKS against, so the kernels that run are the product's (tests/test_gpu_elementwise.py).
#include "elementwise.h"
#include "sctc_diag.h"

extern "C" int sctc_diag_gather_rows(float* dst, int64_t ldd, const float* src, int64_t lds, const int32_t* idx,
                                     int64_t rows, int32_t cols, void* stream)
{
    return sctc::launch_gather_rows(dst, ldd, src, lds, idx, rows, cols, (hipStream_t)stream);
}

extern "C" int sctc_diag_scatter_rows(float* dst, int64_t ldd, const float* src, int64_t lds, const int32_t* idx,
                                      int64_t rows, int32_t cols, void* stream)
{
    return sctc::launch_scatter_rows(dst, ldd, src, lds, idx, rows, cols, (hipStream_t)stream);
}

extern "C" int sctc_diag_add(float* out, const float* a, const float* b, int64_t n, void* stream)
{
    return sctc::launch_add(out, a, b, n, (hipStream_t)stream);
}

extern "C" int sctc_diag_cvt16(const float* src, uint16_t* dst_f16, uint16_t* dst_bf16, int64_t n, void* stream)
{
    return sctc::launch_cvt16(src, dst_f16, dst_bf16, n, (hipStream_t)stream);
}

extern "C" int sctc_diag_add16(float* out, const float* a, const float* b, uint16_t* o_f16, uint16_t* o_bf16,
                               uint16_t* a_bf16, uint16_t* b_bf16, int64_t n, void* stream)
{
    return sctc::launch_add16(out, a, b, o_f16, o_bf16, n, (hipStream_t)stream, a_bf16, b_bf16);
}

extern "C" int sctc_diag_transpose_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int32_t rows,
                                        int32_t cols, void* stream)
{
    return sctc::launch_transpose_bf16(src, ld_src, dst, ld_dst, rows, cols, (hipStream_t)stream);
}

extern "C" int sctc_diag_gather_rows16(float* dst, uint16_t* d_f16, uint16_t* d_bf16, int64_t ldd, const float* src,
                                       int64_t lds, const int32_t* idx, int64_t rows, int32_t cols, void* stream)
{
    return sctc::launch_gather_rows16(dst, d_f16, d_bf16, ldd, src, lds, idx, rows, cols, (hipStream_t)stream);
}
