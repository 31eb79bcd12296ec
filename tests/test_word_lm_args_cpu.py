"""Argument errors of sctc_word_lm_score_workspace_bytes / sctc_word_lm_score_batch / sctc_nbest_rank_words_batch
(csrc/word_lm_score.hip, csrc/lm_score.hip): SCTC_ERR_ARG before a device is touched.  The lexicon
"handle" is a block of zeros: a zeroed handle has 0 words and was built for an alphabet of 0 symbols.  Of the two checks
that read the handle the word range comes first (unk = 2 trips it), and with unk = end = -1 the last check, "a mismatch
with the lexicon's A", rejects every config that got past all the others.  The output and label pointers of the batch
entry are checked before the handle is read."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    _sctc.lib()
    return _sctc


def config(sctc, N=2, A=5, unk=2, end=1, flags=0, U=(3, 2), off=(0, 3), lexicon=True):
    keep = {"lex": ctypes.create_string_buffer(4096),
            "U": np.ascontiguousarray(U if U is not None else [], dtype=np.int32),
            "off": np.ascontiguousarray(off if off is not None else [], dtype=np.int64)}
    cfg = sctc.WordLmScoreConfig(N, A, ctypes.cast(keep["lex"], ctypes.c_void_p) if lexicon else None, unk, end, flags, 0,
                                 sctc.i32(keep["U"]) if U is not None else None,
                                 sctc.i64(keep["off"]) if off is not None else None)
    return cfg, keep


BAD_CONFIGS = {
    "negative N": (dict(N=-1), b"sequences"),
    "A zero": (dict(A=0), b"alphabet"),
    "A beyond 256": (dict(A=257), b"alphabet"),
    "unknown flag": (dict(flags=4), b"flags"),
    "null lexicon": (dict(lexicon=False), b"null lexicon"),
    "unk below -1": (dict(unk=-2), b"below -1"),
    "end below -1": (dict(end=-2), b"below -1"),
    "eos without </s>": (dict(flags=1, end=-1), b"</s>"),
    "null lengths": (dict(U=None), b"null length"),
    "null offsets": (dict(off=None), b"null length"),
    "U of 8192": (dict(U=(8192, 1)), b"8192 labels"),
    "negative U": (dict(U=(-1, 1)), b"labels"),
    "negative offset": (dict(off=(0, -1)), b"negative offset"),
    "unk beyond the words": (dict(unk=2, end=-1), b"outside 0 words"),
    "end beyond the words": (dict(unk=-1, end=0), b"outside 0 words"),
    "A is not the lexicon's": (dict(unk=-1, end=-1), b"the lexicon was built for 0 symbols"),
    "A is not the lexicon's, empty batch": (dict(N=0, U=None, off=None, unk=-1, end=-1),
                                            b"the lexicon was built for 0 symbols"),
}


@pytest.mark.parametrize("name", sorted(BAD_CONFIGS))
def test_word_lm_score_argument_errors(sctc, name):
    L = sctc.lib()
    kw, message = BAD_CONFIGS[name]
    cfg, keep = config(sctc, **kw)
    n = ctypes.c_size_t(77)
    assert L.sctc_word_lm_score_workspace_bytes(ctypes.byref(cfg), ctypes.byref(n)) == -1, name
    assert n.value == 0 and message in L.sctc_last_error(), L.sctc_last_error()
    out = np.zeros(64, dtype=np.float64)
    p = out.ctypes.data                            # never written: the call fails first
    assert L.sctc_word_lm_score_batch(ctypes.byref(cfg), p, p, p, p, p, p, p, 1 << 30, None) == -1, name
    assert message in L.sctc_last_error() and not out.any()
    del keep


def test_word_lm_score_null_pointers(sctc):
    L = sctc.lib()
    n = ctypes.c_size_t(0)
    assert L.sctc_word_lm_score_workspace_bytes(None, ctypes.byref(n)) == -1 and b"null config" in L.sctc_last_error()
    cfg, keep = config(sctc)
    assert L.sctc_word_lm_score_workspace_bytes(ctypes.byref(cfg), None) == -1 and b"null bytes" in L.sctc_last_error()
    assert L.sctc_word_lm_score_batch(None, None, None, None, None, None, None, None, 0, None) == -1
    with pytest.raises(ValueError):
        sctc.check(L.sctc_word_lm_score_batch(None, None, None, None, None, None, None, None, 0, None), "word_lm_score")
    assert L.sctc_abi_version() == 6
    del keep


def test_word_lm_score_null_device_pointers(sctc):
    """NULL sums, counts, status or labels: told before the handle is read; with every
    pointer given the same config gets as far as the handle's own checks"""
    L = sctc.lib()
    cfg, keep = config(sctc, unk=-1, end=-1)
    out = np.zeros(64, dtype=np.float64)
    p = out.ctypes.data

    def call(labels=p, sums=p, counts=p, status=p, c=cfg):
        return L.sctc_word_lm_score_batch(ctypes.byref(c), labels, None, None, sums, counts, status, p, 1 << 30, None)
    for kw in (dict(sums=None), dict(counts=None), dict(status=None)):
        assert call(**kw) == -1 and b"null sums / counts / status" in L.sctc_last_error(), kw
    assert call(labels=None) == -1 and b"null labels" in L.sctc_last_error()
    assert call() == -1 and b"the lexicon was built for 0 symbols" in L.sctc_last_error()
    # rows without labels need no labels array: the call gets past that check
    empty, keep2 = config(sctc, unk=-1, end=-1, U=(0, 0), off=(0, 0))
    assert call(labels=None, c=empty) == -1 and b"the lexicon was built for 0 symbols" in L.sctc_last_error()
    assert call(sums=None, c=empty) == -1 and b"null sums" in L.sctc_last_error()
    assert not out.any()
    del keep, keep2


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    fields = ["N", "A", "lexicon", "unk", "end", "flags", "reserved", "U_b", "label_off"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\nint main(void){printf("%zu", '
                    'sizeof(sctc_word_lm_score_config));\n'
                    + "".join('printf(" %%zu", offsetof(sctc_word_lm_score_config, %s));\n' % f for f in fields)
                    + 'printf(" %d %d\\n", SCTC_WORD_LM_EOS, SCTC_WORD_LM_NO_FINAL_WORD); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    C = sctc.WordLmScoreConfig
    assert got == [ctypes.sizeof(C)] + [getattr(C, f).offset for f in fields] + [sctc.WORD_LM_EOS,
                                                                                 sctc.WORD_LM_NO_FINAL_WORD]


def rank(sctc, B=2, K=3, K_b=(3, 1), U=(1, 2, 3, 4, 5, 6), ptr=True, words=(True, True, True)):
    L = sctc.lib()
    kb = np.ascontiguousarray(K_b, dtype=np.int32) if K_b is not None else None
    u = np.ascontiguousarray(U, dtype=np.int32) if U is not None else None
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data if ptr else None
    w = [buf.ctypes.data if on else None for on in words]
    rc = L.sctc_nbest_rank_words_batch(B, K, sctc.i32(kb) if kb is not None else None,
                                       sctc.i32(u) if u is not None else None, 1.0, 0.0, p, p, None, None, w[0], w[1],
                                       w[2], 1.0, 0.0, p, p, None)
    assert not buf.any()
    return rc


def test_nbest_rank_words_argument_errors(sctc):
    assert rank(sctc, B=-1) == -1
    assert rank(sctc, K=0) == -1
    assert rank(sctc, K=257, K_b=(3, 1), U=[1] * (2 * 257)) == -1
    assert rank(sctc, K_b=None) == -1
    assert rank(sctc, U=None) == -1
    assert rank(sctc, K_b=(4, 1)) == -1          # K_b outside [0, K]
    assert rank(sctc, K_b=(3, -1)) == -1
    assert rank(sctc, U=(1, 2, -3, 4, 5, 6)) == -1
    assert rank(sctc, ptr=False) == -1           # NULL device pointers
    for missing in range(3):                     # every word array is needed
        assert rank(sctc, words=[i != missing for i in range(3)]) == -1
        assert b"null word-LM array" in sctc.lib().sctc_last_error()
    assert rank(sctc, B=0, K_b=None, U=None, ptr=False, words=(False, False, False)) == 0    # launches nothing


def test_python_surface_checks_before_the_device(sctc):
    import ctc_fast
    for fn in (ctc_fast.word_lm_score_batch, ctc_fast.word_lm_perplexity):
        with pytest.raises(ValueError):
            fn([[2, 3]], object())
