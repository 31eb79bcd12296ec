"""Every kernel of csrc/elementwise.hip launched directly and compared BIT FOR BIT with the float64 models of
tests/elementwise_model.py: the optimizer entries (sctc_axpy, sctc_scale, sctc_sumsq, sctc_sumsq_reg,
sctc_nesterov_step, sctc_nesterov_step_reg) through the public C ABI, the internal launchers (gather_rows,
scatter_rows, add, cvt16, add16, transpose_bf16, gather_rows16) through the test-only door of the diag library
(tools/diag/elementwise_entry.hip -> sctc::launch_* of libsctc_hip.so).

Until now they ran only inside whole training steps of tiny networks, judged by one relative norm: never at a size at
which a grid-stride loop wraps (the production buffer wraps forty times), never with the clip factor or the no-L2
ranges in isolation, never with a shadow compared with the rounding it claims to be.  Here the optimizer data sit on a
grid on which fp32 is exact in any order (tests/test_elementwise_model_cpu.py proves that for every case, and that every
listed mutation of the models changes what some case expects); the launchers move or round values, so they are exact
for any input and get the values at which a 16-bit rounding can go wrong (ties both ways, the overflow thresholds, the
denormal ranges of both formats, fp32 denormals, zeros, infinities, NaN -- NaN outputs compared as "is NaN").

Every buffer a launch may write has a sentinel guard on both sides and is compared WHOLE, guard and padding included;
the inputs are compared afterwards too.  The float4 kernels (add, cvt16, add16) are given 16-byte aligned pointers
only: the engine's allocations guarantee that alignment, and misalignment of them is not covered.  Not covered either:
element counts from 2^31, the stream argument's ordering, the softmax and argmax kernels (tests of their own).

One pass per optimizer entry uses standard normal data and non-dyadic coefficients, since grids cannot see rounding:
|got - ref64| <= k x 2^-24 x (sum of the absolute values of the terms of that element), k the number of fp32
roundings on the kernel's path, counted where the bound is formed.

OBSERVED (MI355X)
-----------------
Every exact comparison holds bit for bit, fp32 denormal inputs included: the device rounds them to bfloat16 as IEEE
nearest-even does (0x00008000 -> 0, 0x00008001 -> 0x0001, 0x00018000 -> 0x0002) and adds them without flushing.
Worst |got - ref64| / bound of the real-data pass (n = 525365, one grid wrap):

entry           buffer   k    ratio
axpy            w        2    0.499
scale           w        1    0.995
nesterov        v        4    0.483
nesterov        w        5    0.520
nesterov_reg    v        8    0.243
nesterov_reg    w        9    0.279
sumsq           out      -    0         (equal to math.fsum of the squares)
sumsq_reg       out      5    1.9e-4

Each test takes under two seconds; the production-layout launches (21.3 M floats) 1.6 s each, model included.
"""
import math

import numpy as np
import pytest

from tests import elementwise_model as em
from tests.test_gpu_bf16x3 import print      # noqa: A004  also appends to the suite's test_notes.txt

pytestmark = pytest.mark.gpu

GUARD = 64                  # elements on each side: 256 / 128 bytes, so the payload keeps the allocation's 16-byte alignment
SENTINEL = {np.dtype(np.float32): em.SENT, np.dtype(np.uint16): em.SENT16, np.dtype(np.float64): np.float64(-31337.0),
            np.dtype(np.int32): np.int32(-1), np.dtype(np.uint8): np.uint8(0xA5)}
WS_BYTES = 8192             # sizeof(double) * SS_BLOCKS
ERR_WORKSPACE = -3


@pytest.fixture(scope="module")
def mods():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import _sctc
    from tools.diag import sctc_diag
    return _sctc, sctc_diag.lib(), torch


class Buf(object):
    """a device buffer: `payload` between two sentinel guards, `off` more elements in front (misalignment)"""

    def __init__(self, torch, payload, off=0):
        p = np.ascontiguousarray(payload)
        self.n, self.lo, self.u16 = p.size, GUARD + off, p.dtype == np.uint16
        h = np.full(self.lo + p.size + GUARD, SENTINEL[p.dtype], dtype=p.dtype)
        h[self.lo:self.lo + p.size] = p.reshape(-1)
        self.host0 = h
        self.dev = torch.from_numpy(h.view(np.int16) if self.u16 else h.copy()).cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.lo * self.host0.itemsize

    def image(self):
        a = self.dev.cpu().numpy()
        return a.view(np.uint16) if self.u16 else a

    def expected(self, payload=None):
        h = self.host0.copy()
        if payload is not None:
            h[self.lo:self.lo + self.n] = np.asarray(payload).reshape(-1)
        return h


def ptr(b):
    return None if b is None else b.ptr


def _mismatch(name, got, want, kind=None):
    if got.dtype == np.float32:
        same = em.same32(got, want)
    elif kind in ("f16", "bf16"):
        same = em.same16(got, want, kind)
    else:
        same = got == want
    if same.all():
        return None
    bad = np.flatnonzero(~same)
    i = int(bad[0])
    return "%s: %d of %d elements differ, first at %d (payload starts at %d): got %r, want %r" % (
        name, len(bad), same.size, i, GUARD, got[i], want[i])


def _check(fails, case, bufs, want, kinds=None):
    """bufs: name -> Buf; want: name -> new payload (absent / None = must be unchanged)"""
    for k, b in bufs.items():
        if b is None:
            continue
        msg = _mismatch(k, b.image(), b.expected(want.get(k)), (kinds or {}).get(k))
        if msg:
            fails.append("%s: %s" % (case, msg))


def _report(fails, n):
    assert not fails, "%d mismatches over %d cases:\n%s" % (len(fails), n, "\n".join(fails[:40]))


# ---------------------------------------------------------------- the optimizer entries (public ABI)

def _launch_opt(mods, c, d, ranges="case", n_ranges=None, ws_bytes=WS_BYTES):
    """one launch of case c on host data d -> (rc, bufs); bufs hold every buffer the entry was given"""
    _sctc, _, torch = mods
    L = _sctc.lib()
    b = {"w": Buf(torch, d.w, c.off), "v": Buf(torch, d.v, c.off), "g": Buf(torch, d.g, c.off)}
    if isinstance(ranges, str):
        ranges = c.ranges
    if n_ranges is None:
        n_ranges = 0 if ranges is None else len(ranges) // 2
    rp = None if ranges is None or len(ranges) == 0 else _sctc.i64(np.ascontiguousarray(ranges, dtype=np.int64))
    k = c.kernel
    if k in ("sumsq", "sumsq_reg"):
        b["out"] = Buf(torch, np.array([SENTINEL[np.dtype(np.float64)]]))
        b["ws"] = Buf(torch, np.full(ws_bytes, 0x5A, dtype=np.uint8))
    if k in ("nesterov", "nesterov_reg") and c.S is not None:
        b["S"] = Buf(torch, np.array([c.S], dtype=np.float64))
    S = ptr(b.get("S"))
    if k == "axpy":
        rc = L.sctc_axpy(b["w"].ptr, b["g"].ptr, c.alpha, c.n, None)
    elif k == "scale":
        rc = L.sctc_scale(b["w"].ptr, c.alpha, c.n, None)
    elif k == "sumsq":
        rc = L.sctc_sumsq(b["g"].ptr, c.n, b["out"].ptr, b["ws"].ptr, ws_bytes, None)
    elif k == "sumsq_reg":
        rc = L.sctc_sumsq_reg(b["g"].ptr, b["w"].ptr, b["v"].ptr if c.vel else None, c.mom, c.grad_scale, c.reg, c.n, rp,
                              n_ranges, b["out"].ptr, b["ws"].ptr, ws_bytes, None)
    elif k == "nesterov":
        rc = L.sctc_nesterov_step(b["w"].ptr, b["v"].ptr, b["g"].ptr, c.n, c.mom, c.alpha, c.max_gnorm, c.grad_scale, S,
                                  None)
    else:
        assert k == "nesterov_reg", k
        rc = L.sctc_nesterov_step_reg(b["w"].ptr, b["v"].ptr, b["g"].ptr, c.n, c.mom, c.alpha, c.max_gnorm,
                                      c.grad_scale, c.reg, rp, n_ranges, S, None)
    torch.cuda.synchronize()
    return rc, b


def _opt_exact(mods, kernel, production):
    _sctc, _, _ = mods
    fails, n = [], 0
    for c in em.optimizer_cases():
        if c.kernel != kernel or c.production != production:
            continue
        d = em.optimizer_data(c)
        rc, b = _launch_opt(mods, c, d)
        assert rc == 0, (c.name, _sctc.lib().sctc_last_error())
        want = em.optimizer_model(c, d)             # exact: asserts that every intermediate is a float32
        ws = b.pop("ws", None)
        if ws is not None:                          # the workspace itself is scratch; its guards are not
            img = ws.image()
            if not ((img[:ws.lo] == 0xA5).all() and (img[ws.lo + ws.n:] == 0xA5).all()):
                fails.append("%s: wrote outside the workspace" % c.name)
        if "out" in want:
            want = {"out": np.array([want["out"]])}             # the float64 result IS the exact sum
        else:
            want = {k: x.astype(np.float32) for k, x in want.items()}
        _check(fails, c.name, b, want)
        n += 1
    assert n > 0
    _report(fails, n)


@pytest.mark.parametrize("kernel", sorted(em.OPT_MUTATIONS))
def test_optimizer_entry_bit_exact(mods, kernel):
    """every case of the table but the production one: sizes around the block and the grid cap and far beyond it,
    pointers aligned to 4 bytes only, clip taken / not taken / absent with grad_scale != 1, every kind of no-L2 range"""
    _opt_exact(mods, kernel, production=False)


@pytest.mark.parametrize("kernel", ["nesterov_reg", "sumsq_reg"])
def test_optimizer_entry_bit_exact_at_the_production_layout(mods, kernel):
    """one launch over the cfg-3 flat buffer (21 M floats, forty wraps of the grid) with the bias ranges of
    NNet.noreg_ranges"""
    _opt_exact(mods, kernel, production=True)


def test_production_layout_is_what_a_model_reports(mods):
    """the layout function behind the production case against a live (small) model: buffer size and NNet.noreg_ranges"""
    from nnets import brnnet
    D, A, H, NL, TL = 45, 7, 40, 3, 2
    net = brnnet.NNet(D, A, H, NL, 16, temporalLayer=TL, reg=0.1)
    net._allocate()
    n, ranges = em.production_layout(D, H, NL, A)
    assert net._params.numel() == n
    assert net.noreg_ranges().tolist() == ranges.tolist() and len(ranges) == 2 * (NL + 1)


def test_optimizer_entries_reject_without_writing(mods):
    """bad range lists -> the argument error; a workspace one byte short -> SCTC_ERR_WORKSPACE; nothing is written"""
    _sctc, _, _ = mods
    by = {c.name: c for c in em.optimizer_cases()}
    fails, n = [], 0
    for k in ("nesterov_reg", "sumsq_reg"):
        c = by["%s-ranges-edges" % k]
        d = em.optimizer_data(c)
        for name, nr, flat in em.BAD_RANGES:
            rc, b = _launch_opt(mods, c, d, ranges=flat, n_ranges=nr)
            assert rc == -1, (k, name, rc)
            _check(fails, "%s %s" % (k, name), b, {})
            n += 1
    for k in ("sumsq", "sumsq_reg"):
        c = by["%s-n257" % k]
        rc, b = _launch_opt(mods, c, em.optimizer_data(c), ws_bytes=WS_BYTES - 1)
        assert rc == ERR_WORKSPACE, (k, rc)
        _check(fails, "%s short workspace" % k, b, {})
        n += 1
    _report(fails, n)


def _real_case(kernel):
    return em._opt(kernel, "real", em.PASS + 1000 + 77, "standard normal data, non-dyadic coefficients", mom=0.9,
                   alpha=1e-3, max_gnorm=3.0, grad_scale=1.0 / 3.0, reg=0.05, S=1234.5,
                   ranges=em.edge_ranges(em.PASS + 1077) if kernel.endswith("_reg") else np.zeros(0, dtype=np.int64))


@pytest.mark.parametrize("kernel", sorted(em.OPT_MUTATIONS))
def test_optimizer_entry_rounding_on_real_data(mods, kernel):
    _sctc, _, _ = mods
    c = _real_case(kernel)
    d = em.optimizer_data(c, real=True)
    rc, b = _launch_opt(mods, c, d)
    assert rc == 0, _sctc.lib().sctc_last_error()
    ref = em.optimizer_model(c, d, "f64", exact=False)
    w, v, g = (np.abs(x.astype(np.float64)) for x in (d.w, d.v, d.g))
    mom, gs, reg = (float(np.float32(x)) for x in (c.mom, c.grad_scale, c.reg))
    u = 2.0 ** -24
    ratios = {}
    if kernel == "sumsq":
        # float32 squares are exact in float64 and the terms are non-negative: any summation order is within n 2^-53 fsum
        x = d.g.astype(np.float64)
        fs = math.fsum(x * x)
        k, ratios["out"] = None, abs(float(b["out"].image()[GUARD]) - fs) / (c.n * 2.0 ** -53 * fs)
    elif kernel == "sumsq_reg":
        # t = gs*g + reg_i*(w + mom*vel) in float32: mom*vel, + w, reg_i *, gs*g, + : k = 5 roundings, each at most
        # 2^-24 T with T = |gs g| + reg_i (|w| + |mom vel|) >= |t|.  d(t^2) <= 2 |t| dt + dt^2 <= (2 k 2^-24 + (k 2^-24)^2) T^2;
        # the double sum of the squares adds at most n 2^-53 of itself (non-negative terms).  The bound sums T^2 over
        # ALL elements while the roundings largely cancel in the sum, so the observed ratio is ~2e-4: this pass only
        # guards against gross rounding loss (a relative error near 1e-4 would still pass); the bit-exact cases on the
        # grid carry the weight for this entry.
        k = 5
        regi = np.where(em.inside_ranges(c.n, c.ranges), 0.0, reg)
        T = gs * g + regi * (w + mom * v)
        bound = (2 * k * u + (k * u) ** 2) * math.fsum(T * T) + c.n * 2.0 ** -53 * ref["out"]
        ratios["out"] = abs(float(b["out"].image()[GUARD]) - ref["out"]) / bound
    else:
        if kernel == "axpy":            # y + alpha*x: the product, the sum: k = 2
            k, terms = {"w": 2}, {"w": w + abs(float(np.float32(c.alpha))) * g}
        elif kernel == "scale":         # alpha*x: k = 1
            k, terms = {"w": 1}, {"w": abs(float(np.float32(c.alpha))) * w}
        elif kernel == "nesterov":
            # v' = mom*v - ga*g: ga = alph*grad_scale (a float32 product, exact in the model), mom*v, ga*g, the
            # difference: k = 4;  w' = w + v': one more, k = 5.  (alph itself is formed in double and cast once, in
            # the model exactly as in the kernel.)
            alph = em.clip_alpha(c.alpha, c.max_gnorm, c.grad_scale, c.S, "plain")
            assert alph < float(np.float32(c.alpha))                    # the clip is taken
            tv = mom * v + alph * gs * g
            k, terms = {"v": 4, "w": 5}, {"v": tv, "w": w + tv}
        else:
            # e = gs*g + reg_i*(w + mom*v): mom*v, + w, reg_i *, gs*g, + : 5;  v' = mom*v - alph*e: alph*e, mom*v, the
            # difference: k = 8;  w' = w + v': k = 9
            alph = em.clip_alpha(c.alpha, c.max_gnorm, c.grad_scale, c.S, "reg")
            assert alph < float(np.float32(c.alpha))
            regi = np.where(em.inside_ranges(c.n, c.ranges), 0.0, reg)
            tv = mom * v + alph * (gs * g + regi * (w + mom * v))
            k, terms = {"v": 8, "w": 9}, {"v": tv, "w": w + tv}
        for name in k:
            got = b[name].image()[b[name].lo:b[name].lo + c.n].astype(np.float64)
            ratios[name] = float((np.abs(got - ref[name]) / (k[name] * u * terms[name])).max())
    # every buffer the entry must not write is unchanged, guards included; of the ones it writes (for the two sums the
    # result and the scratch workspace), the guards
    written = k if isinstance(k, dict) else ("out", "ws")
    fails = []
    _check(fails, c.name, {n_: b_ for n_, b_ in b.items() if n_ not in written}, {})
    for name in written:
        img, sent = b[name].image(), SENTINEL[b[name].host0.dtype]
        if not ((img[:b[name].lo] == sent).all() and (img[b[name].lo + b[name].n:] == sent).all()):
            fails.append("%s: wrote outside %s" % (c.name, name))
    _report(fails, 1)
    for name, r in sorted(ratios.items()):
        print("elementwise, real data, %s %s (n = %d): worst |got - ref64| / bound = %.3g" % (kernel, name, c.n, r))
        assert r <= 1.0, (kernel, name, r)


# ---------------------------------------------------------------- the float4 kernels: add, cvt16, add16

def _f4_call(mods, kernel, n, a, b, bufs):
    _, D, torch = mods
    if kernel == "add":
        rc = D.sctc_diag_add(ptr(bufs["out"]), a.ptr, b.ptr, n, None)
    elif kernel == "cvt16":
        rc = D.sctc_diag_cvt16(a.ptr, ptr(bufs.get("f16")), ptr(bufs.get("bf16")), n, None)
    else:
        rc = D.sctc_diag_add16(ptr(bufs.get("out")), a.ptr, b.ptr, ptr(bufs.get("o_f16")), ptr(bufs.get("o_bf16")),
                               ptr(bufs.get("a_bf16")), ptr(bufs.get("b_bf16")), n, None)
    torch.cuda.synchronize()
    return rc


F4_KINDS = {"f16": "f16", "bf16": "bf16", "o_f16": "f16", "o_bf16": "bf16", "a_bf16": "bf16", "b_bf16": "bf16"}
F4_OUTPUTS = {"add": ("out",), "cvt16": ("f16", "bf16"), "add16": em.ADD16_OUTPUTS}


def _f4_run(mods, kernel, n, present, fails, alloc=None, expect_rc=0):
    """one launch with the outputs named in `present` (the others null); alloc: elements allocated (default n)"""
    _sctc, _, torch = mods
    m = alloc or n
    ha, hb = em.add16_inputs(m, 11 + n % 1000)
    a, b = Buf(torch, ha), Buf(torch, hb)
    bufs = {k: Buf(torch, np.full(m, SENTINEL[np.dtype(np.float32 if k == "out" else np.uint16)])) for k in present}
    rc = _f4_call(mods, kernel, n, a, b, bufs)
    name = "%s n=%d %s" % (kernel, n, "+".join(present) or "none")
    assert rc == expect_rc, (name, rc, _sctc.lib().sctc_last_error())
    want = {}
    if rc == 0 and present:
        img = {k: bufs[k].host0[GUARD:GUARD + m] for k in present}
        if kernel == "add":
            want = {"out": em.add(img["out"], ha, hb, n)}
        elif kernel == "cvt16":
            want = em.cvt16(img, ha, n)
        else:
            want = em.add16(img, ha, hb, n)
    bufs.update(a=a, b=b)
    _check(fails, name, bufs, want, F4_KINDS)


@pytest.mark.parametrize("kernel", ["add", "cvt16", "add16"])
def test_float4_kernels_bit_exact(mods, kernel):
    """sizes around one block of float4 and around one pass of the 2048-block grid, and two passes with a tail; every
    output; the specials at both ends of the buffer and across each pass boundary"""
    fails = []
    for n in em.F4_NS:
        _f4_run(mods, kernel, n, F4_OUTPUTS[kernel], fails)
    _report(fails, len(em.F4_NS))


def test_float4_kernels_nullable_outputs(mods):
    """cvt16: each shadow alone, and none (rc 0, nothing launched); add16: each output alone, all five, and the two
    combinations the engine passes (the fp32 sum null)"""
    fails, n = [], 1028
    for present in (("f16",), ("bf16",), ()):
        _f4_run(mods, "cvt16", n, present, fails)
    for present in em.ADD16_COMBOS:
        _f4_run(mods, "add16", n, present, fails)
    _report(fails, 3 + len(em.ADD16_COMBOS))


def test_float4_kernels_reject_a_count_that_is_no_multiple_of_4(mods):
    fails = []
    for kernel in ("add", "cvt16", "add16"):
        for n in (1, 1026, 1027):
            _f4_run(mods, kernel, n, F4_OUTPUTS[kernel], fails, alloc=1028, expect_rc=-1)
    _report(fails, 9)


# ---------------------------------------------------------------- gather, scatter, transpose

GATHER_KINDS = {"f16": "f16", "bf16": "bf16"}


def _gather16_run(mods, c, present, fails):
    _sctc, D, torch = mods
    src, idx = Buf(torch, c.src), Buf(torch, c.idx)
    bufs = {k: Buf(torch, np.full(c.dst_elems, SENTINEL[np.dtype(np.float32 if k == "dst" else np.uint16)]))
            for k in ("dst",) + tuple(present)}
    rc = D.sctc_diag_gather_rows16(bufs["dst"].ptr, ptr(bufs.get("f16")), ptr(bufs.get("bf16")), c.ldd, src.ptr, c.lds,
                                   idx.ptr, c.rows, c.cols, None)
    torch.cuda.synchronize()
    assert rc == 0, (c.name, _sctc.lib().sctc_last_error())
    img = {k: b.host0[GUARD:GUARD + c.dst_elems] for k, b in bufs.items()}
    want = em.gather_rows16(img, c.ldd, c.src, c.lds, c.idx, c.rows, c.cols)
    bufs.update(src=src, idx=idx)
    _check(fails, "gather_rows16 %s %s" % (c.name, "+".join(present) or "no shadow"), bufs, want, GATHER_KINDS)


def test_gather_rows_bit_exact(mods):
    """rows around four per block and one block beyond 1024 rows; cols around one wave; ldd = ceil64(cols) and larger,
    lds different from it; duplicate and out-of-order indices; NaN behind the source's columns; the zero padding and the
    guards compared with everything else"""
    _sctc, D, torch = mods
    fails, cases = [], em.row_cases()
    for c in cases:
        src, idx = Buf(torch, c.src), Buf(torch, c.idx)
        dst = Buf(torch, np.full(c.dst_elems, em.SENT))
        rc = D.sctc_diag_gather_rows(dst.ptr, c.ldd, src.ptr, c.lds, idx.ptr, c.rows, c.cols, None)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, _sctc.lib().sctc_last_error())
        want = em.gather_rows(dst.host0[GUARD:GUARD + c.dst_elems], c.ldd, c.src, c.lds, c.idx, c.rows, c.cols)
        _check(fails, "gather_rows " + c.name, {"dst": dst, "src": src, "idx": idx}, {"dst": want})
    _report(fails, len(cases))


def test_gather_rows16_bit_exact(mods):
    """the same shapes with both shadows; at two shapes every present / absent combination of the two"""
    fails, cases = [], em.row_cases()
    for c in cases:
        _gather16_run(mods, c, ("f16", "bf16"), fails)
    for c in (em.row_case(5, 65, 31), em.row_case(1025, 63, 32)):
        for present in ((), ("f16",), ("bf16",)):
            _gather16_run(mods, c, present, fails)
    _report(fails, len(cases) + 6)


def test_scatter_rows_bit_exact(mods):
    """the same rows and cols; idx a permutation of a destination two rows larger (duplicates would race); the rows no
    index names and the columns from cols on keep their sentinel"""
    _sctc, D, torch = mods
    fails, cases = [], em.row_cases(scatter=True)
    for c in cases:
        src, idx = Buf(torch, c.src), Buf(torch, c.idx)
        dst = Buf(torch, np.full(c.dst_elems, em.SENT))
        rc = D.sctc_diag_scatter_rows(dst.ptr, c.ldd, src.ptr, c.lds, idx.ptr, c.rows, c.cols, None)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, _sctc.lib().sctc_last_error())
        want = em.scatter_rows(dst.host0[GUARD:GUARD + c.dst_elems], c.ldd, c.src, c.lds, c.idx, c.rows, c.cols)
        _check(fails, "scatter_rows " + c.name, {"dst": dst, "src": src, "idx": idx}, {"dst": want})
    _report(fails, len(cases))


def test_transpose_bf16_bit_exact(mods):
    """the engine's padded shapes with its leading dimensions, and ragged extents 1, 31, 33, 95 in each dimension with
    both leading dimensions larger than the extent: the slack of every destination row keeps its sentinel"""
    _sctc, D, torch = mods
    fails, cases = [], em.transpose_cases()
    for c in cases:
        src = Buf(torch, c.src)
        dst = Buf(torch, np.full(c.cols * c.ldd, em.SENT16))
        rc = D.sctc_diag_transpose_bf16(src.ptr, c.lds, dst.ptr, c.ldd, c.rows, c.cols, None)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, _sctc.lib().sctc_last_error())
        want = em.transpose_bf16(dst.host0[GUARD:GUARD + c.cols * c.ldd], c.ldd, c.src, c.lds, c.rows, c.cols)
        _check(fails, "transpose_bf16 " + c.name, {"dst": dst, "src": src}, {"dst": want}, {"dst": "bf16"})
    _report(fails, len(cases))
