"""Argument errors of sctc_ctc_bestpath_batch and sctc_log_rows return before any device call: they are
checked here on a machine without a GPU, as tests/test_abi.py does for the other entries.  The pointers
handed over are never dereferenced by a call that is rejected (or that has nothing to launch)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(0x1000)      # stands for a device pointer; never followed


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


def config(sctc, B=1, A=4, dtype=None, drop=(0,), n_drop=None, ld=None, T=(3,), off=(0,)):
    Tb = np.ascontiguousarray(T, dtype=np.int32)
    fo = np.ascontiguousarray(off, dtype=np.int64)
    cfg = sctc.BestPathConfig(B, A, sctc.F32 if dtype is None else dtype, len(drop) if n_drop is None else n_drop,
                              (ctypes.c_int32 * 16)(*drop), A if ld is None else ld, sctc.i32(Tb), sctc.i64(fo))
    cfg._keep = (Tb, fo)
    return cfg


def call(sctc, cfg, rows=FAKE, ids=FAKE, lens=FAKE, spans=None, scores=None):
    return sctc.lib().sctc_ctc_bestpath_batch(ctypes.byref(cfg) if cfg is not None else None, rows, ids, lens, spans,
                                              scores, None)


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(sctc_bestpath_config),'
                    ' offsetof(sctc_bestpath_config, drop), offsetof(sctc_bestpath_config, ld),'
                    ' offsetof(sctc_bestpath_config, T_b), offsetof(sctc_bestpath_config, frame_off)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    C = sctc.BestPathConfig
    assert got == [ctypes.sizeof(C), C.drop.offset, C.ld.offset, C.T_b.offset, C.frame_off.offset]


def test_bestpath_argument_errors_need_no_gpu(sctc):
    L = sctc.lib()
    assert call(sctc, None) == -1 and b"null config" in L.sctc_last_error()
    ok = config(sctc)
    assert call(sctc, ok, ids=None) == -1 and b"null" in L.sctc_last_error()
    assert call(sctc, ok, lens=None) == -1
    assert call(sctc, ok, rows=None) == -1 and b"null rows" in L.sctc_last_error()
    assert call(sctc, config(sctc, B=-1)) == -1
    assert call(sctc, config(sctc, A=0, ld=4)) == -1
    assert call(sctc, config(sctc, A=4, ld=3)) == -1 and b"ld" in L.sctc_last_error()
    assert call(sctc, config(sctc, n_drop=-1)) == -1
    assert call(sctc, config(sctc, n_drop=17)) == -1 and b"dropped" in L.sctc_last_error()
    assert call(sctc, config(sctc, T=(-1,))) == -1 and b"frames" in L.sctc_last_error()
    assert call(sctc, config(sctc, off=(-5,))) == -1 and b"offset" in L.sctc_last_error()
    assert call(sctc, config(sctc, B=2, T=(3, -2), off=(0, 3))) == -1
    for dtype in (sctc.F16, sctc.BF16, 7, -1):
        assert call(sctc, config(sctc, dtype=dtype)) == -1 and b"dtype" in L.sctc_last_error()
    null_arrays = sctc.BestPathConfig(1, 4, sctc.F32, 0, (ctypes.c_int32 * 16)(), 4, None, None)
    assert call(sctc, null_arrays) == -1
    with pytest.raises(ValueError):
        sctc.check(call(sctc, config(sctc, A=4, ld=3)), "bestpath")


def test_bestpath_empty_batch_is_ok_and_launches_nothing(sctc):
    empty = sctc.BestPathConfig(0, 4, sctc.F64, 1, (ctypes.c_int32 * 16)(0), 4, None, None)
    assert call(sctc, empty, rows=None) == 0
    # the checks of the sizes still apply to an empty batch
    bad = sctc.BestPathConfig(0, 4, sctc.F64, 1, (ctypes.c_int32 * 16)(0), 3, None, None)
    assert call(sctc, bad) == -1


def test_bestpath_map_override_is_checked(sctc):
    os.environ["SCTC_BESTPATH_MAP"] = "sideways"
    try:
        assert call(sctc, config(sctc)) == -1 and b"SCTC_BESTPATH_MAP" in sctc.lib().sctc_last_error()
    finally:
        del os.environ["SCTC_BESTPATH_MAP"]


def test_log_rows_argument_errors_need_no_gpu(sctc):
    L = sctc.lib()
    assert L.sctc_log_rows(FAKE, FAKE, -1, 4, 4, None) == -1
    assert L.sctc_log_rows(FAKE, FAKE, 2, 0, 4, None) == -1
    assert L.sctc_log_rows(FAKE, FAKE, 2, 5, 4, None) == -1 and b"log_rows" in L.sctc_last_error()
    assert L.sctc_log_rows(None, FAKE, 2, 4, 4, None) == -1
    assert L.sctc_log_rows(FAKE, None, 2, 4, 4, None) == -1
    assert L.sctc_log_rows(None, None, 0, 4, 4, None) == 0       # nothing to do


def test_python_surface_checks_before_the_device(sctc):
    import torch
    import ctc_fast
    from new_decoder import decoder
    from nnets import brnnet
    assert callable(ctc_fast.decode_best_path_batch) and callable(ctc_fast.edit_distance_device)
    assert callable(ctc_fast.log_rows) and callable(decoder.ArgmaxDecoder.decode_batch)
    assert callable(brnnet.NNet.forwardDevice) and callable(brnnet.NNet.evaluate)
    y = [np.zeros((4, 3))]
    with pytest.raises(ValueError):
        ctc_fast.decode_best_path_batch(y, drop=range(1, 18))            # 18 symbols with the blank
    with pytest.raises(ValueError):
        ctc_fast.decode_best_path_batch([])
    with pytest.raises(ValueError):
        ctc_fast.decode_best_path_batch(torch.zeros((3, 4)))            # a tensor needs lengths
    if not torch.cuda.is_available():
        with pytest.raises(sctc.SctcError):                              # no fall-back to the host
            ctc_fast.decode_best_path_batch(y)
