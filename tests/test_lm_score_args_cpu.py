"""Argument errors of sctc_lm_score_workspace_bytes / sctc_lm_score_batch / sctc_nbest_rank_batch (csrc/lm_score.hip):
SCTC_ERR_ARG before a device is touched.  The LM "handle" is a block of zeros: no check below may get as far as
believing it (a zeroed handle has an empty vocabulary, so even the symbol-map check rejects the call)."""
import ctypes
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    _sctc.lib()
    return _sctc


def config(sctc, N=2, A=5, kind=0, U=(3, 2), off=(0, 3), lm=True, sym=True, reserved=0, sym_ids=None):
    keep = {"lm": ctypes.create_string_buffer(4096),
            "sym": np.asarray(sym_ids if sym_ids is not None else np.arange(A if A > 0 else 1), dtype=np.int32),
            "U": np.ascontiguousarray(U if U is not None else [], dtype=np.int32),
            "off": np.ascontiguousarray(off if off is not None else [], dtype=np.int64)}
    cfg = sctc.LmScoreConfig(N, A, kind, reserved, ctypes.cast(keep["lm"], ctypes.c_void_p) if lm else None,
                             sctc.i32(keep["sym"]) if sym else None,
                             sctc.i32(keep["U"]) if U is not None else None,
                             sctc.i64(keep["off"]) if off is not None else None)
    return cfg, keep


BAD_CONFIGS = {
    "negative N": dict(N=-1),
    "A zero": dict(A=0),
    "A beyond 256": dict(A=257),
    "unknown kind": dict(kind=3),
    "negative kind": dict(kind=-1),
    "reserved": dict(reserved=1),
    "null lm": dict(lm=False),
    "null symbol map": dict(sym=False),
    "null lengths": dict(U=None),
    "null offsets": dict(off=None),
    "U beyond 8191": dict(U=(8192, 1)),
    "negative U": dict(U=(-1, 1)),
    "negative offset": dict(off=(0, -1)),
    # an n-gram id beyond a byte; the zeroed handle of a neural LM has no vocabulary at all
    "symbol map outside the LM": dict(sym_ids=(0, 1, 300, 2, 3)),
}


@pytest.mark.parametrize("name", sorted(BAD_CONFIGS))
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_lm_score_argument_errors(sctc, name, kind):
    L = sctc.lib()
    kw = dict(kind=kind)
    kw.update(BAD_CONFIGS[name])
    cfg, keep = config(sctc, **kw)
    n = ctypes.c_size_t(77)
    assert L.sctc_lm_score_workspace_bytes(ctypes.byref(cfg), 0, ctypes.byref(n)) == -1, name
    assert n.value == 0 and L.sctc_last_error()
    out = np.zeros(64, dtype=np.float64)
    p = out.ctypes.data                            # never written: the call fails first
    assert L.sctc_lm_score_batch(ctypes.byref(cfg), p, p, p, p, p, 1 << 30, None) == -1, name
    assert not out.any()
    del keep


def test_lm_score_null_pointers(sctc):
    L = sctc.lib()
    n = ctypes.c_size_t(0)
    assert L.sctc_lm_score_workspace_bytes(None, 0, ctypes.byref(n)) == -1
    cfg, keep = config(sctc)
    assert L.sctc_lm_score_workspace_bytes(ctypes.byref(cfg), 0, None) == -1
    assert L.sctc_lm_score_batch(None, None, None, None, None, None, 0, None) == -1
    with pytest.raises(ValueError):
        sctc.check(L.sctc_lm_score_batch(None, None, None, None, None, None, 0, None), "lm_score")
    del keep


def rank(sctc, B=2, K=3, K_b=(3, 1), U=(1, 2, 3, 4, 5, 6), ptr=True):
    L = sctc.lib()
    kb = np.ascontiguousarray(K_b, dtype=np.int32) if K_b is not None else None
    u = np.ascontiguousarray(U, dtype=np.int32) if U is not None else None
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data if ptr else None
    rc = L.sctc_nbest_rank_batch(B, K, sctc.i32(kb) if kb is not None else None, sctc.i32(u) if u is not None else None,
                                 1.0, 0.0, p, p, None, None, p, p, None)
    assert not buf.any()
    return rc


def test_nbest_rank_argument_errors(sctc):
    assert rank(sctc, B=-1) == -1
    assert rank(sctc, K=0) == -1
    assert rank(sctc, K=257, K_b=(3, 1), U=[1] * (2 * 257)) == -1
    assert rank(sctc, K_b=None) == -1
    assert rank(sctc, U=None) == -1
    assert rank(sctc, K_b=(4, 1)) == -1          # K_b outside [0, K]
    assert rank(sctc, K_b=(3, -1)) == -1
    assert rank(sctc, U=(1, 2, -3, 4, 5, 6)) == -1
    assert rank(sctc, ptr=False) == -1           # NULL device pointers
    assert b"nbest_rank" in sctc.lib().sctc_last_error()
    assert rank(sctc, B=0, K_b=None, U=None, ptr=False) == 0     # B == 0 launches nothing, asks for nothing
    assert sctc.lib().sctc_abi_version() == 6
