"""ctypes loader of tools/diag/libsctc_diag.so (hardware probes and the test-only GEMM entry; not the product
library)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsctc_diag.so")
_lib = None


class GemmArgs(ctypes.Structure):
    """sctc_diag_gemm_args of sctc_diag.h: sctc::GemmArgs (csrc/gemm_f32.h) field for field"""
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p),
                ("lda", ctypes.c_int64), ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64),
                ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
                ("a_kcontig", ctypes.c_int32), ("b_kcontig", ctypes.c_int32),
                ("idx_a", ctypes.c_void_p), ("idx_b", ctypes.c_void_p),
                ("bias", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("ldmask", ctypes.c_int64),
                ("addend", ctypes.c_void_p), ("ldadd", ctypes.c_int64),
                ("add_scale", ctypes.c_float), ("relu", ctypes.c_int32), ("accumulate", ctypes.c_int32),
                ("colsum_a", ctypes.c_void_p),
                ("splitk_ws", ctypes.c_void_p), ("splits", ctypes.c_int32),
                ("prec", ctypes.c_int32), ("in16", ctypes.c_int32),
                ("C16a", ctypes.c_void_p), ("C16b", ctypes.c_void_p), ("ldc16", ctypes.c_int64),
                ("skip_c32", ctypes.c_int32),
                ("mask16", ctypes.c_void_p), ("ldmask16", ctypes.c_int64),
                ("A2", ctypes.c_void_p), ("a_sum", ctypes.c_void_p)]


class GemmPlan(ctypes.Structure):
    """sctc_diag_gemm_plan_out of sctc_diag.h: sctc::GemmPlan (csrc/gemm_plan.h) without the template selectors"""
    _fields_ = [(n, ctypes.c_int32) for n in ("kernel", "bm", "bn", "bk", "threads", "occ", "lds_bytes", "grid_x", "splits",
                                              "split_tile_differs")] + [("ws_floats", ctypes.c_int64)]


def gemm_plan(M, N, K, lay, prec, in16, gather=False, a2=False):
    """the product's plan for a GEMM of this shape, layout ("NT": A K-contiguous, B K-contiguous; "TN": both
    row-contiguous) and precision with leading dimensions that are multiples of 8, under the current environment"""
    P = 0x10000                 # a 16-byte aligned address that is never dereferenced
    akc, bkc = int(lay[0] == "N"), int(lay[1] == "T")
    a = GemmArgs(A=P, B=P, C=P, lda=8, ldb=8, ldc=8, M=M, N=N, K=K, a_kcontig=akc, b_kcontig=bkc, splits=1, prec=prec, in16=in16,
                 idx_a=P if gather and not akc else None, idx_b=P if gather and not bkc else None, A2=P if a2 else None)
    out = GemmPlan()
    rc = lib().sctc_diag_gemm_plan(ctypes.byref(a), ctypes.byref(out))
    assert rc == 0
    return out


def lib():
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401  (same HIP runtime instance as the product library)
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        f32p = ctypes.POINTER(ctypes.c_float)
        L.sctc_diag_last_error.restype = ctypes.c_char_p
        L.sctc_selftest.argtypes = [ctypes.c_void_p]
        L.sctc_probe_fabric.argtypes = [f32p, ctypes.c_int32, ctypes.c_void_p]
        L.sctc_probe_mfma.argtypes = [f32p, ctypes.c_int32, ctypes.c_void_p]
        L.sctc_diag_spin.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
        L.sctc_probe_handoff.argtypes = [f32p, ctypes.c_int32, ctypes.c_void_p]
        L.sctc_diag_stream_cu_mask.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int32,
                                               ctypes.POINTER(ctypes.c_void_p)]
        L.sctc_diag_stream_destroy.argtypes = [ctypes.c_void_p]
        L.sctc_diag_where.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_void_p]
        L.sctc_diag_gemm.argtypes = [ctypes.POINTER(GemmArgs), ctypes.c_void_p]
        L.sctc_diag_gemm_plan.argtypes = [ctypes.POINTER(GemmArgs), ctypes.POINTER(GemmPlan)]
        L.sctc_diag_gemm_plan_splits.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)]
        L.sctc_diag_gemm_plan_splits.restype = ctypes.c_int64
        # the internal launchers of csrc/elementwise.h (elementwise_entry.hip); pointers as plain addresses
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
        L.sctc_diag_gather_rows.argtypes = [vp, i64, vp, i64, vp, i64, i32, vp]
        L.sctc_diag_scatter_rows.argtypes = [vp, i64, vp, i64, vp, i64, i32, vp]
        L.sctc_diag_add.argtypes = [vp, vp, vp, i64, vp]
        L.sctc_diag_cvt16.argtypes = [vp, vp, vp, i64, vp]
        L.sctc_diag_add16.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp]
        L.sctc_diag_transpose_bf16.argtypes = [vp, i64, vp, i64, i32, i32, vp]
        L.sctc_diag_gather_rows16.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, i32, vp]
        _lib = L
    return _lib
