"""Every operand and epilogue option of GemmArgs (csrc/gemm_f32.h), on every GEMM implementation, launched directly
through the test-only entry of the diag library (tools/diag/gemm_entry.hip -> sctc::launch_gemm_f32 of
libsctc_hip.so) and compared BIT FOR BIT with the float64 model tests/gemm_model.py.

The public sctc_gemm_f32 / sctc_gemm_h16 reach layout, bias and ReLU only; mask / mask16, addend, accumulate, the
fused column sums, the K-row gathers, the two-addend operand with a_sum, the 16-bit shadows, skip_c32 and an
explicit split-K count ran only inside NNet.costAndGrad, judged by one relative norm per gradient tensor.  Here
(tests/gemm_cases.py) the data sit on an integer grid on which every fp32 summation order is exact
(tests/test_gemm_model_cpu.py proves that for every case, and that every case notices every mutation of the model),
so each comparison is torch.equal.  Operand buffers carry NaN in their padding, in the rows past K and in rows no
gather index names; every output buffer is compared WHOLE -- padding, slack and sentinels included; the split-K
workspace is exactly splits * M * (N + 1) floats, NaN-filled, followed by a sentinel guard.

One pass per implementation uses standard normal data instead (integers cannot see rounding), within the bound
this project uses for direct GEMM checks: |got - ref64| <= 2e-6 (6e-7 for the bf16x3 kernel) x (sum|a||b| + |bias| +
|add_scale addend| + |C_prev|); the worst ratios are printed through the notes helper of tests/test_gpu_bf16x3.py.

Not covered: column sums taken by EVERY N tile instead of the first -- the extra blocks store the same value (or
the same split-K partial), and with accumulate they race on one read-modify-write, so on the device that mistake shows
only when two such blocks happen not to overlap; the 32-bit product row x ld of the gathered loads,
(uint32_t)ia * (uint32_t)lda, which needs an operand above 16 GiB to overflow."""
import ctypes

import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import gemm_model as gm
from tests.test_gpu_bf16x3 import print      # noqa: A004  also appends to the suite's test_notes.txt

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import _sctc
    from tools.diag import sctc_diag
    return _sctc.lib(), sctc_diag, torch


def _select(monkeypatch, impl):
    for n in gc.ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    for n, v in gc.IMPLS[impl]["env"].items():
        monkeypatch.setenv(n, v)


def _launch(mods, c, d):
    """one launch of case c on the host data d; returns (splits used, device images of everything it may write)"""
    L, diag, torch = mods
    D = diag.lib()
    im = gc.IMPLS[c.impl]
    t16 = torch.float16 if im["prec"] == 1 else torch.bfloat16

    def dev(x, op16=False):
        if x is None:
            return None
        if x.dtype == np.uint16:
            return torch.from_numpy(x.view(np.int16).copy()).cuda()
        t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        return t.to(t16) if op16 else t            # integers and pre-rounded values: the conversion is exact

    def ptr(t, byte_off=0):
        return None if t is None else t.data_ptr() + byte_off

    in16 = bool(im["in16"])
    A, B, A2 = dev(d.A, in16), dev(d.B, in16), dev(d.A2, in16)
    ia, ib = dev(d.idx_a), dev(d.idx_b)
    bias, mask, mask16, addend = dev(d.bias_buf), dev(d.mask), dev(d.mask16), dev(d.addend)
    out = dict(C=dev(d.C0), C16a=dev(d.C16a0), C16b=dev(d.C16b0), colsum=dev(d.colsum0), asum=dev(d.asum0))
    splits, ws_floats = c.splits, c.splits * c.M * (c.N + 1)
    if "planner" in c.opts:
        p = diag.gemm_plan(c.M, c.N, c.K, c.lay, im["prec"], im["in16"], "gather" in c.opts, "a2" in c.opts)
        splits, ws_floats = p.splits, p.ws_floats
        assert splits > 1 and ws_floats == splits * c.M * (c.N + 1), (c.name, splits, ws_floats)
    ws = None
    if splits > 1:
        ws = torch.full((ws_floats + GUARD,), float("nan"), device="cuda")
        ws[ws_floats:] = gc.SENT
    a = diag.GemmArgs(
        A=ptr(A), B=ptr(B), C=ptr(out["C"]), lda=d.A.shape[1], ldb=d.B.shape[1], ldc=d.ldc, M=c.M, N=c.N, K=c.K,
        a_kcontig=d.akc, b_kcontig=d.bkc, idx_a=ptr(ia), idx_b=ptr(ib), bias=ptr(bias, 4 * d.bias_off),
        mask=ptr(mask), ldmask=0 if d.mask is None else d.mask.shape[1],
        addend=ptr(addend), ldadd=0 if d.addend is None else d.addend.shape[1], add_scale=gc.ADD_SCALE,
        relu=int("relu" in c.opts), accumulate=int("acc" in c.opts), colsum_a=ptr(out["colsum"]),
        splitk_ws=ptr(ws), splits=splits, prec=im["prec"], in16=im["in16"],
        C16a=ptr(out["C16a"]), C16b=ptr(out["C16b"]), ldc16=d.ldc16, skip_c32=int("skip" in c.opts),
        mask16=ptr(mask16), ldmask16=0 if d.mask16 is None else d.mask16.shape[1], A2=ptr(A2), a_sum=ptr(out["asum"]))
    rc = D.sctc_diag_gemm(ctypes.byref(a), None)
    assert rc == 0, (c.name, L.sctc_last_error())
    torch.cuda.synchronize()
    if ws is not None:
        assert bool((ws[ws_floats:] == gc.SENT).all()), c.name + ": wrote past the split-K workspace"
    host = {}
    for k, t in out.items():
        if t is not None:
            h = t.cpu().numpy()
            host[k] = h.view(np.uint16) if h.dtype == np.int16 else h
    return splits, host


def _mismatch(name, got, want):
    if got.dtype.kind == "f":
        same = (got == want) | (np.isnan(got) & np.isnan(want))
    else:
        same = got == want
    if same.all():
        return None
    bad = np.argwhere(~same)
    i = tuple(bad[0])
    return "%s: %d of %d elements differ, first at %s: got %r, want %r" % (name, len(bad), same.size, i, got[i], want[i])


@pytest.mark.parametrize("impl", sorted(gc.IMPLS))
def test_gemm_options_bit_exact(mods, monkeypatch, impl):
    """the whole case table of one implementation; every image bit-equal, every guard region intact"""
    _select(monkeypatch, impl)
    failures, n = [], 0
    for c in gc.cases_for(impl):
        d = gc.host_data(c)
        splits, got = _launch(mods, c, d)
        want = gc.expected_images(c, d, gm.gemm_model(gc.model_args(c, d, splits=splits)))
        for k in got:
            msg = _mismatch(k, got[k], getattr(want, k))
            if msg:
                failures.append("%s (splits %d): %s" % (c.name, splits, msg))
        n += 1
    assert not failures, "%d of %d cases:\n%s" % (len({f.split(" ")[0] for f in failures}), n, "\n".join(failures[:40]))


def test_planner_leaves_the_last_slice_empty_and_the_kernels_cope(mods, monkeypatch):
    """fp32, 128 x 128 tiles: 76 output tiles, K = 1296 = 81 K tiles of 16 -> 10 slices of 9 tiles, slice 9 starts at
    tile 81.  The same K and count on a small output are in every fp32 table (...-TN-...x1296-s10-...)."""
    _, diag, _ = mods
    monkeypatch.setenv("SCTC_GEMM_SHAPE", "0")
    s = diag.gemm_plan(19 * 128, 4 * 128, 1296, "TN", 0, 0).splits
    assert s == 10 and (s - 1) * ((81 + s - 1) // s) >= 81
    for impl in ("f32_shape0", "f32_shape1", "f32_shape2", "f32_shape3"):
        assert any(c.K == 1296 and c.splits == 10 for c in gc.cases_for(impl))


def _real_cases(impl):
    im = gc.IMPLS[impl]
    BM, BN, BK = im["tile"]
    M, N, K = 3 * BM, 3 * BN, 4 * BK + 4
    K8 = (K + 7) // 8 * 8
    wg = "colsum addend acc" + (" a2 asum" if im["prec"] == 0 else "")
    if im["prec"] in (1, 2):
        delta = gc._case(impl, "NT" if im["in16"] else "NN", M, N, K8, 1, "mask c16a c16b")
    else:
        delta = gc._case(impl, "NN", M, N, K8, 1, "mask")
    return [gc._case(impl, "TN", M, N, K, 3, wg), gc._case(impl, "TN", M, N, K, 1, wg), delta]


@pytest.mark.parametrize("impl", sorted(gc.IMPLS))
def test_gemm_options_real_data(mods, monkeypatch, impl):
    """standard normal data at the 3 x 3-tile shape: the weight-gradient and the delta option sets"""
    _select(monkeypatch, impl)
    im = gc.IMPLS[impl]
    tol = 6e-7 if im["prec"] == 3 else 2e-6
    worst = 0.0
    for c in _real_cases(impl):
        d = gc.host_data(c, real=True)
        splits, got = _launch(mods, c, d)
        g = gc.model_args(c, d, splits=splits)
        ref = gm.gemm_model(g)
        M, N, K = c.M, c.N, c.K
        A = gm._logical(d.A, d.akc, None, M, K).astype(np.float32)
        if d.A2 is not None:
            A = A + gm._logical(d.A2, d.akc, None, M, K).astype(np.float32)
        B = gm._logical(d.B, d.bkc, None, N, K).astype(np.float32)
        if im["prec"] in (1, 2) and not im["in16"]:
            rnd = gm.round_f16 if im["prec"] == 1 else gm.round_bf16
            Ar, Br = rnd(A), rnd(B)
        else:
            Ar, Br = A.astype(np.float64), B.astype(np.float64)
        bound = np.abs(Ar) @ np.abs(Br).T
        if d.addend is not None:
            bound = bound + np.abs(gc.ADD_SCALE * d.addend[:M, :N].astype(np.float64))
        if "acc" in c.opts:
            bound = bound + np.abs(d.C0[:M, :N].astype(np.float64))
        C = got["C"]
        ratio = float((np.abs(C[:M, :N].astype(np.float64) - ref.C) / bound).max())
        if "mask" in c.opts:                # a masked element is exactly zero
            dead = ~(d.mask[:M, :N] > 0)
            assert (C[:M, :N][dead] == 0).all(), c.name
        if "colsum" in c.opts:
            cb = np.abs(A.astype(np.float64)).sum(axis=1) + np.abs(d.colsum0[:M].astype(np.float64))
            ratio = max(ratio, float((np.abs(got["colsum"][:M].astype(np.float64) - ref.colsum_a) / cb).max()))
            assert (got["colsum"][M:] == gc.SENT).all(), c.name
        print("gemm options, real data, %s: worst |got - ref64| / bound = %.2e (bound %.0e)" % (c.name, ratio, tol))
        worst = max(worst, ratio)
        # everything outside the logical region still holds its sentinel; exact by-products are bit-equal
        assert (C[M:] == gc.SENT).all() and (C[:, N:] == gc.SENT).all(), c.name
        if "asum" in c.opts:
            want = gc.expected_images(c, d, ref).asum
            assert _mismatch("a_sum", got["asum"], want) is None, c.name
        C32 = np.ascontiguousarray(C[:M, :N])
        for k, bits in (("C16a", gm.f16_bits), ("C16b", gm.bf16_bits)):
            if k in got:        # the shadows: the nearest-even rounding of the fp32 C the same launch stored
                assert np.array_equal(got[k][:M, :N], bits(C32)), c.name + " " + k
                assert (got[k][M:] == gc.SENT16).all() and (got[k][:, N:] == gc.SENT16).all(), c.name
        assert ratio <= tol, (c.name, ratio)
    assert worst <= tol
