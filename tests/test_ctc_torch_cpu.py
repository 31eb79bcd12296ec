"""ctc_torch without a GPU: every argument error of ctc_torch.ctc_loss is raised on the host, the three C entries
behind it (sctc_ctc_tnc_probs / _empty / _grad) return SCTC_ERR_ARG before any device call, and the host helpers --
targets -> concatenated labels, lengths and offsets; reduction -> per-utterance scale -- are held against
torch.nn.functional.ctc_loss on CPU float64 tensors.  The pointers handed to a rejected call (or to one with nothing to
launch) are never followed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(0x1000)      # stands for a device pointer; never followed


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


# ---------------------------------------------------------------- the C entries

def config(sctc, T=4, N=2, C=5, dtype=None, mode=0, blank=0, strides=None):
    st = strides or (N * C, C, 1)
    return sctc.TncConfig(T, N, C, sctc.F32 if dtype is None else dtype, mode, blank, *st)


def calls(sctc):
    L = sctc.lib()
    ref = lambda c: ctypes.byref(c) if c is not None else None
    return {
        "probs": lambda c, a=FAKE, b=FAKE, d=FAKE: L.sctc_ctc_tnc_probs(ref(c), a, b, d, None),
        "empty": lambda c, a=FAKE, b=FAKE, d=FAKE, n=1: L.sctc_ctc_tnc_empty(ref(c), a, b, d, None, n, FAKE, FAKE, FAKE, None),
        "grad": lambda c, a=FAKE, b=FAKE, d=FAKE: L.sctc_ctc_tnc_grad(ref(c), a, b, FAKE, FAKE, FAKE, d, None),
    }


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(sctc_tnc_config),'
                    ' offsetof(sctc_tnc_config, blank), offsetof(sctc_tnc_config, stride_t),'
                    ' offsetof(sctc_tnc_config, stride_n), offsetof(sctc_tnc_config, stride_c),'
                    ' SCTC_TNC_LOG_PROBS, SCTC_TNC_LOGITS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    C = sctc.TncConfig
    assert got == [ctypes.sizeof(C), C.blank.offset, C.stride_t.offset, C.stride_n.offset, C.stride_c.offset,
                   sctc.TNC_LOG_PROBS, sctc.TNC_LOGITS]


@pytest.mark.parametrize("entry", ["probs", "empty", "grad"])
def test_tnc_argument_errors_need_no_gpu(sctc, entry):
    L = sctc.lib()
    call = calls(sctc)[entry]
    assert call(None) == -1 and b"null config" in L.sctc_last_error()
    for first in (0, 1, 2):                      # a NULL pointer with work to do
        ptrs = [FAKE, FAKE, FAKE]
        ptrs[first] = None
        assert call(config(sctc), *ptrs) == -1 and b"null pointer" in L.sctc_last_error()
    assert call(config(sctc, T=-1)) == -1
    assert call(config(sctc, N=-1)) == -1
    assert call(config(sctc, C=0)) == -1 and b"alphabet" in L.sctc_last_error()
    assert call(config(sctc, blank=-1)) == -1 and b"blank" in L.sctc_last_error()
    assert call(config(sctc, blank=5)) == -1
    for dtype in (sctc.F16, sctc.BF16, 7, -1):
        assert call(config(sctc, dtype=dtype)) == -1 and b"dtype" in L.sctc_last_error()
    for mode in (2, -1):
        assert call(config(sctc, mode=mode)) == -1 and b"mode" in L.sctc_last_error()
    # rowbase is int32: T * N must fit
    assert call(config(sctc, T=1 << 16, N=1 << 15)) == -1 and b"int32" in L.sctc_last_error()
    assert call(config(sctc, T=(1 << 31) - 1, N=2)) == -1
    with pytest.raises(ValueError):
        sctc.check(call(config(sctc, C=0)), entry)


@pytest.mark.parametrize("entry", ["probs", "empty", "grad"])
def test_tnc_nothing_to_do_launches_nothing(sctc, entry):
    call = calls(sctc)[entry]
    assert call(config(sctc, T=0), None, None, None) == 0
    listed = {"n": 0} if entry == "empty" else {}     # of N == 0 utterances none can be listed
    assert call(config(sctc, N=0), None, None, None, **listed) == 0
    # the checks of the sizes still apply
    assert call(config(sctc, T=0, C=0), None, None, None) == -1
    assert call(config(sctc, N=0, blank=9), None, None, None, **listed) == -1


def test_tnc_empty_list_length_is_checked(sctc):
    L = sctc.lib()
    call = calls(sctc)["empty"]
    assert call(config(sctc), n=-1) == -1 and b"listed" in L.sctc_last_error()
    assert call(config(sctc, N=2), n=3) == -1
    assert call(config(sctc), None, None, None, n=0) == 0          # no utterance with an empty target


# ---------------------------------------------------------------- argument errors of the Python surface

def good(T=6, N=3, C=5, S=4, dtype=torch.float64):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, N, C, generator=g, dtype=dtype)
    targets = torch.randint(1, C, (N, S), generator=g)
    return x, targets, [T, T - 1, T - 2], [2, 1, 3]


def test_argument_errors_are_raised_before_the_gpu(ct, sctc):
    x, tg, il, tl = good()
    T, N, C = x.shape
    with pytest.raises(ValueError, match="dimensions"):
        ct.ctc_loss(x[0], tg, il, tl)                                   # wrong rank
    with pytest.raises(ValueError, match="dimensions"):
        ct.ctc_loss(x[None], tg, il, tl)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            ct.ctc_loss(x.to(dt), tg, il, tl)
    with pytest.raises(TypeError):
        ct.ctc_loss(x.to(torch.int32), tg, il, tl)                      # wrong dtype
    for bad in ([T + 1, 3, 3], [0, 3, 3], [T, -1, 3]):
        with pytest.raises(ValueError, match="input_lengths"):
            ct.ctc_loss(x, tg, bad, tl)
    for bad in ([5, 1, 1], [1, -1, 1]):
        with pytest.raises(ValueError, match="target"):
            ct.ctc_loss(x, tg, il, bad)                                 # outside [0, S]
    with pytest.raises(ValueError, match="input_lengths"):
        ct.ctc_loss(x, tg, [T, T], tl)                                  # not one entry per utterance
    with pytest.raises(ValueError, match="target_lengths"):
        ct.ctc_loss(x, tg, il, torch.tensor([1, 1, 1, 1]))
    with pytest.raises(ValueError, match="concatenated"):
        ct.ctc_loss(x, torch.tensor([1, 2, 3, 1, 2]), il, tl)           # 5 labels for lengths that sum to 6
    for bad in (-1, C, C + 3):
        with pytest.raises(ValueError, match="blank"):
            ct.ctc_loss(x, tg, il, tl, blank=bad)
    with pytest.raises(ValueError, match="reduction"):
        ct.ctc_loss(x, tg, il, tl, reduction="average")
    with pytest.raises(ValueError, match="reduction"):
        ct.CTCLoss(reduction="average")
    for bad in (-1, C, C + 7):
        t2 = tg.clone()
        t2[2, 2] = bad                                                  # inside target_lengths[2] == 3
        with pytest.raises(ValueError, match="label"):
            ct.ctc_loss(x, t2, il, tl)
        with pytest.raises(ValueError, match="label"):
            ct.ctc_loss(x, torch.cat([t2[n, :u] for n, u in enumerate(tl)]), il, tl)
    with pytest.raises(TypeError):
        ct.ctc_loss(x, tg.double(), il, tl)
    with pytest.raises(ValueError):
        ct.ctc_loss(x, tg[:2], il, tl)                                  # two rows of targets for three utterances
    if not torch.cuda.is_available():
        with pytest.raises(sctc.SctcError):                             # valid arguments: no fall-back to the host
            ct.ctc_loss(x, tg, il, tl)
        with pytest.raises(sctc.SctcError):
            ct.CTCLoss()(x, tg, il, tl)


def test_padding_is_not_validated(ct):
    """entries beyond target_lengths[n] are never read: -1 and C + 7 there are legal"""
    x, tg, il, tl = good()
    C = x.shape[2]
    t2 = tg.clone()
    t2[0, 2:] = -1
    t2[1, 1:] = C + 7
    labels, U, off = ct._host_targets(t2, tl, 3, C)
    assert labels.tolist() == tg[0, :2].tolist() + tg[1, :1].tolist() + tg[2, :3].tolist()
    assert U.tolist() == tl and off.tolist() == [0, 2, 3]
    cat = torch.cat([torch.cat([tg[n, :u] for n, u in enumerate(tl)]), torch.tensor([-1, C + 7])])
    labels2, U2, off2 = ct._host_targets(cat, torch.tensor(tl), 3, C)     # a tail beyond the sum is padding too
    assert labels2.tolist() == labels.tolist() and U2.tolist() == tl and off2.tolist() == [0, 2, 3]
    assert labels.dtype == np.int32 and U.dtype == np.int32 and off.dtype == np.int64


def test_ctc_fast_does_not_import_ctc_torch(sctc):
    code = ("import sys; sys.path[:0] = [%r, %r]; import ctc_fast; assert 'ctc_torch' not in sys.modules"
            % (ROOT, os.path.join(ROOT, "stanford-ctc_amd")))
    subprocess.check_call([sys.executable, "-c", code])


# ---------------------------------------------------------------- the host helpers against PyTorch's CPU loss

CASES = [  # (T, C, input lengths, target lengths): an empty target, unequal lengths, a single utterance
    (7, 5, [7, 4, 6], [3, 1, 2]),
    (6, 4, [6, 5, 6, 3], [2, 0, 3, 1]),
    (5, 6, [5], [2]),
    (4, 3, [4, 2], [0, 0]),
]


def oracle(T, C, il, tl, seed=0):
    g = torch.Generator().manual_seed(seed)
    N, S = len(il), max(max(tl), 1)
    lp = torch.randn(T, N, C, generator=g, dtype=torch.float64).log_softmax(2).requires_grad_()
    tg = torch.randint(1, C, (N, S), generator=g)
    return lp, tg


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("concatenated", [False, True])
def test_host_targets_against_pytorch(ct, case, concatenated):
    """PyTorch's CPU loss on the helper's (labels, U, off), utterance by utterance, equals its loss on the original
    targets: the helper cuts the labels where PyTorch does"""
    T, C, il, tl = case
    lp, tg = oracle(T, C, il, tl)
    N = len(il)
    given = torch.cat([tg[n, :u] for n, u in enumerate(tl)]) if concatenated else tg
    want = F.ctc_loss(lp, given, torch.tensor(il), torch.tensor(tl), reduction="none")
    labels, U, off = ct._host_targets(given.to(torch.int32) if concatenated else given, tuple(tl), N, C)
    assert U.tolist() == tl and len(labels) == sum(tl)
    for n in range(N):
        mine = torch.from_numpy(labels[off[n]:off[n] + U[n]].astype(np.int64))[None]
        got = F.ctc_loss(lp[:, n:n + 1], mine.reshape(1, -1), torch.tensor(il[n:n + 1]), torch.tensor([int(U[n])]),
                         reduction="none")
        assert got.item() == pytest.approx(want[n].item(), rel=1e-14)


def scale_by_mutant(ct, which):
    """the helpers, or one of two wrong versions of them (the mutation check)"""
    if which == "helper":
        return ct._reduce, ct._scale
    if which == "no clamp":         # divides by target_length itself
        return (lambda l, u, r: ct._reduce(l, u, r) if r != "mean" else (l / u.to(l.dtype)).mean(),
                lambda g, u, r, N: ct._scale(g, u, r, N) if r != "mean" else g.to(torch.float64).reshape(()) / (u.to(torch.float64) * N))
    # averages before dividing: the batch mean over the mean target length
    return (lambda l, u, r: ct._reduce(l, u, r) if r != "mean" else l.mean() / u.clamp(min=1).to(l.dtype).mean(),
            lambda g, u, r, N: ct._scale(g, u, r, N) if r != "mean" else
            (g.to(torch.float64).reshape(()) / (u.clamp(min=1).to(torch.float64).mean() * N)).expand(N))


def reduction_agrees(ct, which, case, reduction):
    T, C, il, tl = case
    reduce, scale = scale_by_mutant(ct, which)
    lp, tg = oracle(T, C, il, tl)
    N = len(il)
    ilt, tlt = torch.tensor(il), torch.tensor(tl)
    weight = torch.linspace(0.5, 2.0, N, dtype=torch.float64) if reduction == "none" else torch.tensor(1.5, dtype=torch.float64)
    want = F.ctc_loss(lp, tg, ilt, tlt, reduction=reduction)
    want_grad, = torch.autograd.grad((want * weight).sum(), lp)
    losses = F.ctc_loss(lp, tg, ilt, tlt, reduction="none")
    got = reduce(losses.detach(), tlt, reduction)
    s = scale(weight, tlt, reduction, N)
    if s.shape != (N,) or s.dtype != torch.float64:
        return False
    got_grad, = torch.autograd.grad(losses, lp, grad_outputs=s.contiguous())
    return bool(torch.allclose(got, want.detach(), rtol=1e-14, atol=0, equal_nan=False)
                and torch.allclose(got_grad, want_grad, rtol=1e-12, atol=1e-15, equal_nan=False))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_reduction_and_scale_against_pytorch(ct, case, reduction):
    """_reduce gives PyTorch's reduced loss, and the [N] losses' gradients weighted by _scale add up to the gradient of
    PyTorch's reduced loss times grad_output"""
    assert reduction_agrees(ct, "helper", case, reduction)


@pytest.mark.parametrize("which", ["no clamp", "averages first"])
def test_wrong_mean_rules_are_caught(ct, which):
    """a helper that divides by target_length without the clamp, or that averages before dividing, fails a case"""
    assert not all(reduction_agrees(ct, which, case, "mean") for case in CASES)
    assert all(reduction_agrees(ct, which, case, r) for case in CASES for r in ("none", "sum"))
