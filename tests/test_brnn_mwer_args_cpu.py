"""The argument errors of the BRNN engine's MWER step (include/sctc.h) that are reachable without a
device -- the scalars of the descriptor are checked before the handle is looked at --, the ctypes mirrors of its two
structs, and the ValueErrors / TypeErrors of the Python surface (NNet.mwerCostAndGradBatch, NNet.nbestBatch, sgd.SGD)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    ge._paths()
    return _sctc


def descriptor(sctc, K=2, scale=1.0, subtract_mean=1, ctc_weight=0.0, null=()):
    K_b = np.array([2], dtype=np.int32)
    lab = np.array([1, 2, 1], dtype=np.int32)
    U = np.array([2, 1], dtype=np.int32)
    W = np.array([1.0, 0.0])
    p = lambda name, arr, f: None if name in null else f(arr)
    mw = sctc.MwerMinibatch(K, p("K_b", K_b, sctc.i32), p("hyp_labels", lab, sctc.i32), p("hyp_U", U, sctc.i32),
                            p("errors", W, lambda a: a.ctypes.data_as(sctc.c_f64p)), scale, subtract_mean, ctc_weight)
    return mw, (K_b, lab, U, W)


def minibatch(sctc):
    T = np.array([5], dtype=np.int32)
    return sctc.Minibatch(1, sctc.i32(T), 0x1000, None, None), T


BAD = [dict(K=0), dict(K=257), dict(K=-3), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
       dict(ctc_weight=-0.5), dict(ctc_weight=float("nan")), dict(ctc_weight=float("inf")), dict(subtract_mean=2),
       dict(subtract_mean=-1), dict(null=("K_b",)), dict(null=("hyp_U",)), dict(null=("errors",))]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join("%s=%s" % (k, v) for k, v in kw.items()))
def test_bad_descriptors_are_refused_without_a_device(sctc, kw):
    L = sctc.lib()
    mw, keep = descriptor(sctc, **kw)
    mb, keep2 = minibatch(sctc)
    need = ctypes.c_size_t(0)
    fake = ctypes.c_void_p(0x1000)          # never followed: the descriptor is checked first
    for rc in (L.sctc_brnn_mwer_cost_and_grad(fake, ctypes.byref(mb), ctypes.byref(mw), 0, None, None, None),
               L.sctc_brnn_mwer_cost_and_grad_async(fake, ctypes.byref(mb), ctypes.byref(mw), 0, None, None),
               L.sctc_brnn_mwer_workspace_bytes(fake, ctypes.byref(mb), ctypes.byref(mw), ctypes.byref(need))):
        assert rc == ARG, kw
        assert L.sctc_last_error().startswith(b"brnn_mwer")


def test_null_arguments(sctc):
    L = sctc.lib()
    mw, keep = descriptor(sctc)
    mb, keep2 = minibatch(sctc)
    need = ctypes.c_size_t(0)
    assert L.sctc_brnn_mwer_cost_and_grad(None, ctypes.byref(mb), ctypes.byref(mw), 0, None, None, None) == ARG
    assert L.sctc_brnn_mwer_cost_and_grad(None, ctypes.byref(mb), None, 0, None, None, None) == ARG
    assert L.sctc_brnn_mwer_cost_and_grad_async(None, ctypes.byref(mb), ctypes.byref(mw), 0, None, None) == ARG
    assert L.sctc_brnn_mwer_workspace_bytes(None, ctypes.byref(mb), ctypes.byref(mw), ctypes.byref(need)) == ARG
    assert L.sctc_brnn_mwer_workspace_bytes(None, ctypes.byref(mb), None, ctypes.byref(need)) == ARG
    assert L.sctc_brnn_set_mwer_workspace(None, None, 0) == ARG


def test_struct_mirrors_match_the_header(sctc, tmp_path):
    fields = {"sctc_mwer_minibatch": sctc.MwerMinibatch, "sctc_mwer_outputs": sctc.MwerOutputs}
    src = ['#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\nint main(void) {']
    for cname, cls in fields.items():
        src.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            src.append('printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        src.append('printf("\\n");')
    src.append("return 0; }")
    c = tmp_path / "m.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "m")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    for line in subprocess.check_output([exe]).decode().splitlines():
        name, size, *offs = line.split()
        cls = fields[name]
        assert int(size) == ctypes.sizeof(cls), name
        assert [int(o) for o in offs] == [getattr(cls, f).offset for f, _ in cls._fields_], name


class FakeNet:
    """NNet's MWER surface up to the first device call: the checks in front of it need no GPU"""

    def __new__(cls):
        from nnets import brnnet
        net = brnnet.NNet.__new__(brnnet.NNet)
        net._h, net.train, net.outputDim, net.inputDim, net.reg = object(), True, 6, 4, 0.0
        return net


def test_python_surface_errors(sctc):
    net = FakeNet()
    data = [np.zeros((4, 5))]
    hyps, errs = [[np.array([1, 2]), np.array([3])]], [np.array([1.0, 0.0])]
    call = net.mwerCostAndGradBatch
    with pytest.raises(ValueError, match="n-best lists"):
        call(data, hyps + hyps, errs)
    with pytest.raises(ValueError, match="hypotheses and"):
        call(data, hyps, [np.array([1.0])])
    with pytest.raises(ValueError, match="scale"):
        call(data, hyps, errs, scale=-1.0)
    with pytest.raises(ValueError, match="scale"):
        call(data, hyps, errs, scale=float("nan"))
    with pytest.raises(TypeError, match="scale"):
        call(data, hyps, errs, scale="1")
    with pytest.raises(ValueError, match="ctc_weight"):
        call(data, hyps, errs, ctc_weight=-0.1)
    with pytest.raises(TypeError, match="ctc_weight"):
        call(data, hyps, errs, ctc_weight=None)
    with pytest.raises(ValueError, match="labels_list"):
        call(data, hyps, errs, ctc_weight=0.5)
    with pytest.raises(ValueError, match="label rows"):
        call(data, hyps, errs, labels_list=[[1], [2]], ctc_weight=0.5)
    with pytest.raises(TypeError, match="integer"):
        call(data, [[np.array([1.5, 2.0]), np.array([3])]], errs)
    with pytest.raises(ValueError, match="outside 1"):
        call(data, [[np.array([1])] * 257], [np.zeros(257)])
    net.train = False
    with pytest.raises(ValueError, match="train=True"):
        call(data, hyps, errs)
    net.train, net._h = True, None
    with pytest.raises(RuntimeError):
        call(data, hyps, errs)
    with pytest.raises(RuntimeError):
        net.mwerCostAndGradBatchAsync(data, hyps, errs)


def test_nbest_batch_errors(sctc):
    net = FakeNet()
    data, refs = [np.zeros((4, 5))], [[1, 2]]
    with pytest.raises(ValueError, match="unit"):
        net.nbestBatch(data, refs, 2, unit="syllable")
    with pytest.raises(ValueError, match="nbest"):
        net.nbestBatch(data, refs, 0, unit="char")
    with pytest.raises(ValueError, match="nbest"):
        net.nbestBatch(data, refs, 257, unit="char")
    with pytest.raises(ValueError, match="space"):
        net.nbestBatch(data, refs, 2, unit="word")
    with pytest.raises(ValueError, match="space"):
        net.nbestBatch(data, refs, 2, unit="word", space=6)
    with pytest.raises(ValueError, match="references"):
        net.nbestBatch(data, refs + refs, 2, unit="char")


def test_sgd_criterion_errors(sctc):
    import sgd
    with pytest.raises(ValueError, match="criterion"):
        sgd.SGD(None, 10, criterion="nope")
    with pytest.raises(ValueError, match="unknown mwer option"):
        sgd.SGD(None, 10, criterion="mwer", mwer=dict(nbset=3))
