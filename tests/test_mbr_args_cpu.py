"""Every SCTC_ERR_ARG of sctc_intern_words_batch / sctc_nbest_mbr_batch (include/sctc.h) is returned
before a device is touched, so it is checked here without one; and the ValueErrors of the Python surface."""
import ctypes

import numpy as np
import pytest

ARG, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def sctc():
    import os
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


def intern_cfg(sctc, U=(3, 2), off=(0, 3), groups=(0, 2), A=8, space=1, N=None, G=None, null=()):
    U = np.array(U, dtype=np.int32)
    off = np.array(off, dtype=np.int64)
    g = np.array(groups, dtype=np.int32)
    keep = (U, off, g)
    cfg = sctc.InternConfig(len(U) if N is None else N, len(g) - 1 if G is None else G, A, space,
                            None if "U_b" in null else sctc.i32(U), None if "label_off" in null else sctc.i64(off),
                            None if "group_off" in null else sctc.i32(g))
    return cfg, keep


def intern_rc(sctc, batch=True, out=(1, 1, 1, 1), **kw):
    cfg, keep = intern_cfg(sctc, **kw)
    L = sctc.lib()
    nbytes = ctypes.c_size_t(123)
    rc = L.sctc_intern_words_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes))
    if rc != 0:
        assert nbytes.value == 0
    if batch:
        # fake non-NULL pointers: every check below fails before a pointer is followed
        ptr = [0x1000 if v else None for v in out]
        rc2 = L.sctc_intern_words_batch(ctypes.byref(cfg), ptr[0], ptr[1], ptr[2], ptr[3], 0x1000, 0, None)
        if rc != 0:
            assert rc2 == rc
        return rc2
    return rc


def test_intern_argument_errors(sctc):
    L = sctc.lib()
    nbytes = ctypes.c_size_t(0)
    assert L.sctc_intern_words_workspace_bytes(None, ctypes.byref(nbytes)) == ARG
    cfg, keep = intern_cfg(sctc)
    assert L.sctc_intern_words_workspace_bytes(ctypes.byref(cfg), None) == ARG
    assert L.sctc_intern_words_batch(None, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 1 << 20, None) == ARG
    for kw in (dict(N=-1), dict(G=-1), dict(A=0), dict(A=257), dict(space=0), dict(space=8), dict(U=(3, -1)),
               dict(U=(3, 4096)), dict(off=(0, -1)), dict(groups=(0, 2, 1, 2)), dict(groups=(1, 2)), dict(groups=(0, 1)),
               dict(null=("U_b",)), dict(null=("label_off",)), dict(null=("group_off",))):
        assert intern_rc(sctc, **kw) == ARG, kw
        assert L.sctc_last_error().startswith(b"intern_words:")
    # missing outputs
    for out in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert intern_rc(sctc, out=out) == ARG, out
    # valid arguments, a workspace that is too small
    assert intern_rc(sctc) == WORKSPACE
    assert intern_rc(sctc, U=(4095, 0), off=(0, 0)) == WORKSPACE
    # nothing to do
    assert intern_rc(sctc, U=(), off=(), groups=(0,)) == 0
    assert intern_rc(sctc, U=(), off=(), groups=(0, 0, 0)) == 0


def test_intern_workspace_bytes(sctc):
    cfg, keep = intern_cfg(sctc, U=(5, 6, 0), off=(0, 5, 11), groups=(0, 2, 3))
    nbytes = ctypes.c_size_t(0)
    assert sctc.lib().sctc_intern_words_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == 0
    # rows | groups | base | meta (6 slots) | table (16 entries): one 256-byte slice each
    assert nbytes.value == 5 * 256


def mbr_cfg(sctc, B=2, K=2, unit=1, flags=0, A=8, space=1, scale=1.0, Kb=(2, 1), U=(3, 2, 4, 0), off=(0, 3, 5, 9), null=()):
    Kb = np.array(Kb, dtype=np.int32)
    U = np.array(U, dtype=np.int32)
    off = np.array(off, dtype=np.int64)
    cfg = sctc.MbrConfig(B, K, unit, flags, A, space, scale, None if "K_b" in null else sctc.i32(Kb),
                         None if "U_b" in null else sctc.i32(U), None if "label_off" in null else sctc.i64(off))
    return cfg, (Kb, U, off)


def mbr_rc(sctc, out=(1,) * 10, ws=0x1000, **kw):
    """labels scores order post risk best mbr_order dist conf conf_len"""
    cfg, keep = mbr_cfg(sctc, **kw)
    L = sctc.lib()
    nbytes = ctypes.c_size_t(123)
    rc = L.sctc_nbest_mbr_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes))
    if rc != 0:
        assert nbytes.value == 0
    ptr = [0x1000 if v else None for v in out]
    rc2 = L.sctc_nbest_mbr_batch(ctypes.byref(cfg), *(ptr + [ws, 0, None]))
    if rc != 0:
        assert rc2 == rc
    return rc2


def test_mbr_argument_errors(sctc):
    L = sctc.lib()
    nbytes = ctypes.c_size_t(0)
    assert L.sctc_nbest_mbr_workspace_bytes(None, ctypes.byref(nbytes)) == ARG
    cfg, keep = mbr_cfg(sctc)
    assert L.sctc_nbest_mbr_workspace_bytes(ctypes.byref(cfg), None) == ARG
    assert L.sctc_nbest_mbr_batch(None, *([0x1000] * 11 + [1 << 20, None])) == ARG
    for kw in (dict(B=-1), dict(K=0), dict(K=257), dict(unit=2), dict(unit=-1), dict(flags=4), dict(flags=-1),
               dict(Kb=(3, 1)), dict(Kb=(2, -1)), dict(U=(3, 2, 4096, 0)), dict(U=(-1, 2, 4, 0)), dict(off=(0, 3, -5, 9)),
               dict(A=0), dict(A=257), dict(space=0), dict(space=8), dict(scale=-0.5), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(null=("K_b",)), dict(null=("U_b",)), dict(null=("label_off",))):
        assert mbr_rc(sctc, **kw) == ARG, kw
        assert L.sctc_last_error().startswith(b"nbest_mbr:")
    # the space is not read in character unit
    assert mbr_rc(sctc, unit=0, space=0) == WORKSPACE
    assert mbr_rc(sctc, unit=0, space=99) == WORKSPACE
    # a length beyond the limit counts even at a rank beyond K_b
    assert mbr_rc(sctc, Kb=(1, 1), U=(3, 5000, 4, 0)) == ARG
    # missing arrays and outputs: labels, scores, post, risk, best, mbr_order; order may be NULL
    for miss in (0, 1, 3, 4, 5, 6):
        out = [1] * 10
        out[miss] = 0
        assert mbr_rc(sctc, out=out) == ARG, miss
    out = [1] * 10
    out[2] = 0
    assert mbr_rc(sctc, out=out) == WORKSPACE
    # the optional outputs are needed exactly with their flags
    for flags, miss, want in ((0, 7, WORKSPACE), (2, 7, ARG), (0, 8, WORKSPACE), (1, 8, ARG), (1, 9, ARG), (0, 9, WORKSPACE)):
        out = [1] * 10
        out[miss] = 0
        assert mbr_rc(sctc, flags=flags, out=out) == want, (flags, miss)
    # valid arguments: short and missing workspace
    assert mbr_rc(sctc) == WORKSPACE and mbr_rc(sctc, ws=None) == WORKSPACE
    assert mbr_rc(sctc, flags=3, scale=0.0) == WORKSPACE
    # nothing to do: no array is looked at
    assert mbr_rc(sctc, B=0, null=("K_b", "U_b", "label_off"), out=(0,) * 10, ws=None) == 0


def test_python_surface_value_errors(sctc):
    import ctc_fast
    hyps = [[[2, 3], [2]]]
    for kw in (dict(unit="phone"), dict(scale=-1.0), dict(scale=float("nan")), dict(unit="word"),
               dict(unit="word", space=0), dict(unit="word", space=300), dict(A=0), dict(A=300, space=1)):
        with pytest.raises(ValueError):
            ctc_fast.mbr_nbest(hyps, [[0.0, 0.0]], **kw)
    for kw in (dict(space=0), dict(space=256), dict(space=3, A=3), dict(space=1, A=500)):
        with pytest.raises(ValueError):
            ctc_fast.intern_words([[2, 3]], [0, 1], **kw)
        with pytest.raises(ValueError):
            ctc_fast.word_errors_batch([[2]], [[2]], **kw)
    with pytest.raises(ValueError):
        ctc_fast.word_errors_batch([[2], [3]], [[2]], 1)
    assert ctc_fast.word_errors_batch([], [], 1).shape == (0, 5)


def test_struct_mirrors(sctc, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(sctc_intern_config),'
                    ' offsetof(sctc_intern_config, group_off), sizeof(sctc_mbr_config), offsetof(sctc_mbr_config, scale),'
                    ' offsetof(sctc_mbr_config, label_off)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(sctc.InternConfig), sctc.InternConfig.group_off.offset, ctypes.sizeof(sctc.MbrConfig),
                   sctc.MbrConfig.scale.offset, sctc.MbrConfig.label_off.offset]
