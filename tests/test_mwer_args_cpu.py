"""The argument checks of the MWER surface, none of which needs a GPU: every ValueError / TypeError of
ctc_torch.mwer_loss, MWERLoss and mwer_nbest is raised on the host before the device is touched, the three C entries
answer SCTC_ERR_ARG for bad values with pointers that lead nowhere, and the ctypes mirror of sctc_mwer_config matches
the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


@pytest.fixture(scope="module")
def ct(sctc):
    import ctc_torch
    return ctc_torch


T, N, K, S, C = 6, 2, 3, 4, 5


def good():
    """a well-formed call on CPU tensors: the only thing wrong with it is the device"""
    return dict(input=torch.zeros(T, N, C).log_softmax(2), hyps=torch.ones(N, K, S, dtype=torch.int64),
                hyp_lengths=torch.full((N, K), 2), errors=torch.zeros(N, K), input_lengths=[6, 5])


def call(ct, **change):
    kw = good()
    kw.update(change)
    return ct.mwer_loss(**kw)


def test_a_well_formed_call_fails_only_on_the_device(ct, sctc):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sctc.SctcError):
        call(ct)
    with pytest.raises(sctc.SctcError):
        call(ct, hyp_counts=[3, 0], errors=np.zeros((N, K), dtype=np.int32), hyp_lengths=[[2, 2, 2], [1, 0, 4]])


TYPE_ERRORS = [
    dict(input=np.zeros((T, N, C))),
    dict(input=torch.zeros(T, N, C, dtype=torch.float16)),
    dict(input=torch.zeros(T, N, C, dtype=torch.bfloat16)),
    dict(input=torch.zeros(T, N, C, dtype=torch.int32)),
    dict(hyps=[[[1]]]),
    dict(hyps=torch.ones(N, K, S)),
    dict(hyps=torch.ones(N, K, S, dtype=torch.bool)),
    dict(hyp_lengths=torch.full((N, K), 2.0)),
    dict(hyp_lengths=[[2.0] * K] * N),
    dict(errors=torch.zeros(N, K, dtype=torch.bool)),
    dict(errors=torch.zeros(N, K, dtype=torch.complex64)),
    dict(input_lengths=torch.tensor([6.0, 5.0])),
    dict(hyp_counts=[3.0, 1.0]),
]

VALUE_ERRORS = [
    dict(input=torch.zeros(T, N)),
    dict(input=torch.zeros(T, N, 0)),
    dict(reduction="avg"),
    dict(blank=C),
    dict(blank=-1),
    dict(scale=-0.5),
    dict(scale=float("inf")),
    dict(scale=float("nan")),
    dict(hyps=torch.ones(N, K, dtype=torch.int64)),
    dict(hyps=torch.ones(N + 1, K, S, dtype=torch.int64)),
    dict(hyps=torch.ones(N, 0, S, dtype=torch.int64), hyp_lengths=torch.zeros(N, 0, dtype=torch.int64),
         errors=torch.zeros(N, 0)),
    dict(hyps=torch.ones(N, 257, 1, dtype=torch.int64), hyp_lengths=torch.ones(N, 257, dtype=torch.int64),
         errors=torch.zeros(N, 257)),
    dict(input_lengths=[6]),
    dict(input_lengths=[6, 0]),
    dict(input_lengths=[7, 5]),
    dict(hyp_counts=[3]),
    dict(hyp_counts=[4, 1]),
    dict(hyp_counts=[-1, 1]),
    dict(hyp_lengths=torch.full((N, K + 1), 2)),
    dict(hyp_lengths=torch.full((N, K), S + 1)),
    dict(hyp_lengths=torch.full((N, K), -1)),
    dict(errors=torch.zeros(N, K + 1)),
    dict(errors=torch.zeros(N * K)),
    dict(hyps=torch.full((N, K, S), C, dtype=torch.int64)),
    dict(hyps=torch.full((N, K, S), -1, dtype=torch.int64)),
    dict(hyps=torch.zeros(N, K, S, dtype=torch.int64)),                     # the blank as a label
    dict(hyps=torch.full((N, K, S), 2, dtype=torch.int64), blank=2),
]


@pytest.mark.parametrize("change", TYPE_ERRORS, ids=lambda c: "-".join(c))
def test_type_errors(ct, change):
    with pytest.raises(TypeError):
        call(ct, **change)


@pytest.mark.parametrize("i", range(len(VALUE_ERRORS)))
def test_value_errors(ct, i):
    with pytest.raises(ValueError):
        call(ct, **VALUE_ERRORS[i])


def test_the_row_index_limit(ct):
    big = torch.zeros(1).expand(2 ** 23, 1, 2)              # no memory behind it
    with pytest.raises(ValueError, match="int32 row index"):
        ct.mwer_loss(big, torch.ones(1, 256, 1, dtype=torch.int64), torch.ones(1, 256, dtype=torch.int64),
                     torch.zeros(1, 256), [4])


def test_slots_the_contract_does_not_read_are_not_validated(ct, sctc):
    """ranks >= K_n, ranks with a non-finite error and one-frame utterances: garbage labels and lengths raise nothing
    -- the call gets as far as the device"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    hyps = torch.ones(N, K, S, dtype=torch.int64)
    lengths = torch.full((N, K), 2)
    errors = torch.zeros(N, K)
    hyps[0, 2] = -1
    lengths[0, 2] = 99                      # beyond hyp_counts[0] = 2
    hyps[0, 1] = C + 3
    errors[0, 1] = float("nan")             # a non-finite error
    hyps[1] = 0
    lengths[1] = -5                         # a one-frame utterance
    with pytest.raises(sctc.SctcError):
        call(ct, hyps=hyps, hyp_lengths=lengths, errors=errors, hyp_counts=[2, 3], input_lengths=[6, 1])
    hyps[0, 0, 1] = C                       # ... and a slot that IS read
    with pytest.raises(ValueError):
        call(ct, hyps=hyps, hyp_lengths=lengths, errors=errors, hyp_counts=[2, 3], input_lengths=[6, 1])


def test_module_and_nbest_arguments(ct):
    with pytest.raises(ValueError):
        ct.MWERLoss(reduction="avg")
    with pytest.raises(ValueError):
        ct.MWERLoss(scale=-1.0)
    crit = ct.MWERLoss(scale=2.0, reduction="sum", subtract_mean=False, logits=True)
    assert (crit.blank, crit.scale, crit.reduction, crit.subtract_mean, crit.logits) == (0, 2.0, "sum", False, True)
    with pytest.raises(ValueError):
        crit(torch.zeros(T, N), torch.ones(N, K, S, dtype=torch.int64), torch.full((N, K), 2), torch.zeros(N, K), [6, 5])
    x = torch.zeros(T, N, C).log_softmax(2)
    refs, rl = torch.ones(N, 3, dtype=torch.int64), [3, 2]
    with pytest.raises(ValueError, match="blank"):
        ct.mwer_nbest(x, [6, 5], refs, rl, 4, unit="char", blank=1)
    for kw in (dict(unit="phone"), dict(unit="word"), dict(unit="word", space=0), dict(unit="word", space=C)):
        with pytest.raises(ValueError):
            ct.mwer_nbest(x, [6, 5], refs, rl, 4, **kw)
    for nbest in (0, 257):
        with pytest.raises(ValueError):
            ct.mwer_nbest(x, [6, 5], refs, rl, nbest, unit="char")
    with pytest.raises(ValueError):
        ct.mwer_nbest(x, [6, 7], refs, rl, 4, unit="char")
    with pytest.raises(ValueError):
        ct.mwer_nbest(x, [6, 5], refs, [3, 4], 4, unit="char")
    with pytest.raises(ValueError):
        ct.mwer_nbest(x, [6, 5], refs[:1], rl, 4, unit="char")


# ---------------------------------------------------------------- the C entries

def cfg(sctc, **change):
    kw = dict(T=T, N=N, K=K, C=C, dtype=sctc.F64, mode=sctc.TNC_LOG_PROBS, stride_t=N * C, stride_n=C, stride_c=1,
              scale=1.0, subtract_mean=1)
    kw.update(change)
    return sctc.MwerConfig(**kw)


def entries(sctc):
    """each entry with every pointer set (to addresses that lead nowhere) and the position of its pointers"""
    L = sctc.lib()
    fake = [ctypes.c_void_p(4096 * (i + 1)) for i in range(12)]
    return [("probs", lambda c, a: L.sctc_ctc_mwer_probs(c, *a, None), fake[:4]),
            ("coef", lambda c, a: L.sctc_ctc_mwer_coef(c, *a, None), fake[:11]),
            ("combine", lambda c, a: L.sctc_ctc_mwer_combine(c, *a, None), fake[:7])]


BAD_CONFIGS = [dict(T=-1), dict(N=-1), dict(K=0), dict(K=257), dict(C=0), dict(dtype=2), dict(dtype=-1), dict(mode=2),
               dict(T=2 ** 20, N=2 ** 5, K=2 ** 6), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
               dict(subtract_mean=2), dict(subtract_mean=-1)]


@pytest.mark.parametrize("change", BAD_CONFIGS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_entries_refuse_bad_configs_without_a_device(sctc, change):
    for name, fn, ptrs in entries(sctc):
        assert fn(ctypes.byref(cfg(sctc, **change)), ptrs) == -1, name
        assert name.encode() in sctc.lib().sctc_last_error()


def test_entries_refuse_null_pointers_and_launch_nothing_for_empty_batches(sctc):
    for name, fn, ptrs in entries(sctc):
        assert fn(None, ptrs) == -1, name
        for i in range(len(ptrs)):
            holed = list(ptrs)
            holed[i] = None
            assert fn(ctypes.byref(cfg(sctc)), holed) == -1, (name, i)
            assert b"null pointer" in sctc.lib().sctc_last_error()
        assert fn(ctypes.byref(cfg(sctc, N=0)), ptrs) == 0, name            # nothing to do: the pointers are not followed
    for name, fn, ptrs in entries(sctc):
        if name != "coef":
            assert fn(ctypes.byref(cfg(sctc, T=0)), ptrs) == 0, name
    assert sctc.lib().sctc_abi_version() == 6


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    fields = [f[0] for f in sctc.MwerConfig._fields_]
    assert fields == ["T", "N", "K", "C", "dtype", "mode", "stride_t", "stride_n", "stride_c", "scale", "subtract_mean"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\nint main(void){printf("%zu", '
                    'sizeof(sctc_mwer_config));\n'
                    + "".join('printf(" %%zu", offsetof(sctc_mwer_config, %s));\n' % f for f in fields)
                    + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(sctc.MwerConfig)] + [getattr(sctc.MwerConfig, f).offset for f in fields]
    assert got == want
    assert sctc.NBEST_MAX_K == 256
