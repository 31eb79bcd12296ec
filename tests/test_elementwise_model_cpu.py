"""CPU-side half of the direct elementwise tests (tests/test_gpu_elementwise.py): the models of
tests/elementwise_model.py against hand-computed values; the precondition that makes the optimizer comparison on the
device BIT-exact -- for every case the exact float64 evaluation, the float32 evaluation and the one with fused
multiply-adds agree bit for bit, and every intermediate is a float32; liveness -- every listed mutation of the models is
noticed by at least one case of the tables; the argument rejections, which launch nothing; and the production layout
against the engine's own tensor table."""
import ctypes
import os

import numpy as np
import pytest

from tests import elementwise_model as em

A64 = em.Arith("f64", exact=True)


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    import _sctc
    from tools.diag import sctc_diag
    if not (os.path.exists(_sctc.LIB_PATH) and os.path.exists(sctc_diag.LIB_PATH)):
        ge.build()
    return _sctc, sctc_diag


# ---------------------------------------------------------------- the models, by hand

def test_rounding_models_by_hand():
    x = np.array([2049, 2051, -2049, 65504, 65519.996, 65520, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 0.0,
                  -0.0, np.inf, 1e-45], dtype=np.float32)
    assert em.f16_bits(x).tolist() == [0x6800, 0x6802, 0xE800, 0x7BFF, 0x7BFF, 0x7C00, 0x0001, 0x0000, 0x0001, 0x0000,
                                       0x8000, 0x7C00, 0x0000]
    assert em.f16_bits(x, "trunc").tolist() == [0x6800, 0x6801, 0xE800, 0x7BFF, 0x7BFF, 0x7BFF, 0x0001, 0x0000, 0x0000,
                                                0x0000, 0x8000, 0x7C00, 0x0000]
    assert em.f16_bits(x, "ties_away").tolist() == [0x6801, 0x6802, 0xE801, 0x7BFF, 0x7BFF, 0x7C00, 0x0001, 0x0001,
                                                    0x0001, 0x0000, 0x8000, 0x7C00, 0x0000]
    y = np.concatenate([np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 3.4028234663852886e38, np.inf],
                                 dtype=np.float32),
                        em._u32(0x7F7F7FFF, 0x7F7F8000, 0x00008000, 0x00008001, 0x00018000, 0x80000001)])
    assert em.bf16_bits(y).tolist() == [0x3F80, 0x3F82, 0xBF80, 0x7F80, 0x7F80, 0x7F7F, 0x7F80, 0x0000, 0x0001, 0x0002,
                                        0x8000]
    assert em.bf16_bits(y, "trunc").tolist() == [0x3F80, 0x3F81, 0xBF80, 0x7F7F, 0x7F80, 0x7F7F, 0x7F7F, 0x0000, 0x0000,
                                                 0x0001, 0x8000]
    assert em.bf16_bits(y, "ties_away").tolist() == [0x3F81, 0x3F82, 0xBF81, 0x7F80, 0x7F80, 0x7F7F, 0x7F80, 0x0001,
                                                     0x0001, 0x0002, 0x8000]
    nans = em._u32(0x7FC00000, 0x7F800001, 0xFFC00000)
    assert em.isnan16(em.bf16_bits(nans), "bf16").all() and em.isnan16(em.f16_bits(nans), "f16").all()
    from oracle.brnn import round_bf16
    assert np.isinf(round_bf16(nans[1:2]))[0]           # why the model has a rounding of its own
    assert em.same16(np.array([0x7FC0], dtype=np.uint16), np.array([0xFFC1], dtype=np.uint16), "bf16").all()
    assert not em.same16(np.array([0x0000], dtype=np.uint16), np.array([0x8000], dtype=np.uint16), "bf16").any()
    assert not em.same32(np.float32([0.0]), np.float32([-0.0])).any() and em.same32(nans[:1], nans[1:2]).all()
    # the models agree with the oracle's roundings wherever those are defined (no NaN)
    from oracle.brnn import round_f16
    d = em.shadow_data(5000, 3)
    d = d[np.isfinite(d)]
    with np.errstate(over="ignore"):
        assert np.array_equal(em.bf16_bits(d).astype(np.uint32) << 16, round_bf16(d).astype(np.float32).view(np.uint32))
        assert np.array_equal(em.f16_bits(d).view(np.float16).astype(np.float64), round_f16(d))


def test_optimizer_models_by_hand():
    w, v, g = np.array([1.0, 2.0]), np.array([4.0, -8.0]), np.array([16.0, 32.0])
    assert em.axpy(A64, w, g, 0.5).tolist() == [9.0, 18.0]
    assert em.scale(A64, w, -0.25).tolist() == [-0.25, -0.5]
    assert em.sumsq(g) == 1280.0
    # clip: sqrt(S) = 64.  nesterov: gnorm = 64 / 4 = 16 > 8 -> alph = 0.5 * 8 / 16 = 0.25, ga = alph / 4 = 1 / 16
    nw, nv = em.nesterov(A64, w, v, g, 0.5, 0.5, 8.0, 0.25, 4096.0)
    assert nv.tolist() == [2.0 - 1.0, -4.0 - 2.0] and nw.tolist() == [2.0, -4.0]
    assert em.clip_alpha(0.5, 8.0, 0.25, 4096.0, "reg") == 0.0625 and em.clip_alpha(0.5, 8.0, 0.25, None, "reg") == 0.5
    assert em.clip_alpha(0.5, 16.0, 0.25, 4096.0, "plain") == 0.5           # 16 > 16 is false: not taken
    # nesterov_reg, element 1 inside a no-L2 range: e = g / 4 + [0.5 * (1 + 0.5 * 4), 0] = [5.5, 8]; alph = 1 / 16
    nw, nv = em.nesterov_reg(A64, w, v, g, 0.5, 0.5, 8.0, 0.25, 0.5, [1, 2], 4096.0)
    assert nv.tolist() == [2.0 - 5.5 / 16, -4.0 - 0.5] and nw.tolist() == [3.0 - 5.5 / 16, -2.5]
    assert em.sumsq_reg(A64, g, w, v, 0.5, 0.25, 0.5, [1, 2]) == 5.5 ** 2 + 8.0 ** 2
    assert em.sumsq_reg(A64, g, w, None, 0.5, 0.25, 0.5, [1, 2]) == 4.5 ** 2 + 8.0 ** 2
    assert em.sumsq_reg(A64, g, w, v, 0.5, 0.25, 0.5, [1, 2], "vel_ignored") == 4.5 ** 2 + 8.0 ** 2
    assert em.inside_ranges(6, [0, 1, 2, 2, 3, 4, 4, 6]).tolist() == [True, False, False, True, True, True]
    assert em.inside_ranges(6, [1, 3], "range_beg_exclusive").tolist() == [False, False, True, False, False, False]
    assert em.inside_ranges(6, [1, 3], "range_end_inclusive").tolist() == [False, True, True, True, False, False]
    with pytest.raises(AssertionError):
        em.axpy(A64, np.array([1.0]), np.array([1.0 + 2.0 ** -23]), 2.0 ** -3)        # off the grid: the model says so


def test_layout_models_by_hand():
    S = em.SENT
    src = np.array([1, 2, 9, 3, 4, 9, 5, 6, 9], dtype=np.float32)          # 3 rows, lds 3, cols 2
    idx = np.array([2, 0, 2], dtype=np.int32)
    d0 = np.full(12, S, dtype=np.float32)
    assert em.gather_rows(d0, 4, src, 3, idx, 3, 2).tolist() == [5, 6, 0, 0, 1, 2, 0, 0, 5, 6, 0, 0]
    assert em.gather_rows(d0, 4, src, 3, idx, 3, 2, "gather_padding_unwritten").tolist() == [5, 6, S, S, 1, 2, S, S, 5, 6,
                                                                                           S, S]
    assert em.scatter_rows(d0, 4, src, 3, np.array([2, 0], dtype=np.int32), 2, 2).tolist() == [3, 4, S, S, S, S, S, S, 1,
                                                                                             2, S, S]
    t0 = np.full(8, em.SENT16, dtype=np.uint16)
    one, two, three = 0x3F80, 0x4000, 0x4040
    got = em.transpose_bf16(t0, 4, np.array([1, 2, 3, 9, 2, 3, 1, 9], dtype=np.float32), 4, 2, 2)       # 2 x 2 of ld 4
    assert got.tolist() == [one, two, em.SENT16, em.SENT16, two, three, em.SENT16, em.SENT16]
    a = np.array([1, 2, 3, 4], dtype=np.float32)
    b = np.array([0.5, 0.5, -3, 2.0 ** -8], dtype=np.float32)
    img = {k: np.zeros(4, dtype=np.float32 if k == "out" else np.uint16) for k in ("out", "o_bf16", "a_bf16")}
    got = em.add16(img, a, b, 4)
    assert got["out"].tolist() == [1.5, 2.5, 0.0, 4 + 2.0 ** -8] and got["o_f16"] is None and got["b_bf16"] is None
    assert got["o_bf16"].tolist() == [0x3FC0, 0x4020, 0x0000, 0x4080] and got["a_bf16"].tolist() == [one, two, three, 0x4080]
    assert em.add16(img, a, b, 4, "add16_input_shadows_swapped")["a_bf16"].tolist() == [0x3F00, 0x3F00, 0xC040, 0x3B80]


# ---------------------------------------------------------------- the optimizer table: exactness

def _same(a, b):
    if set(a) != set(b):
        return False
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


@pytest.mark.parametrize("kernel", sorted(em.OPT_MUTATIONS))
def test_optimizer_cases_are_exact_in_fp32(kernel):
    """the data lie on the stated grid, and the three evaluations agree bit for bit (the exact one also asserts that
    every intermediate is a float32): no summation order, contraction or rounding mode can change a bit on the device"""
    n_cases = 0
    for c in em.optimizer_cases():
        if c.kernel != kernel:
            continue
        d = em.optimizer_data(c)
        for x in (d.w, d.v, d.g):
            assert x.dtype == np.float32 and np.array_equal(np.round(x * 16), x * 16), c.name
            assert np.abs(x).max(initial=0.0) <= 64, c.name
        for p in (c.mom, c.alpha, c.max_gnorm, c.grad_scale, c.reg):
            assert np.frexp(p)[0] == 0.5, (c.name, p)                   # a power of two
        if c.S is not None:
            assert np.frexp(c.S)[0] == 0.5 and np.frexp(c.S)[1] % 2 == 1, (c.name, c.S)      # a power of four
        exact = em.optimizer_model(c, d, "f64", exact=True)
        assert _same(exact, em.optimizer_model(c, d, "f32")), c.name
        assert _same(exact, em.optimizer_model(c, d, "fma")), c.name
        for k, x in exact.items():
            if k != "out":
                assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), c.name
        n_cases += 1
    assert n_cases >= 8


def test_clip_cases_tell_the_two_rules_apart():
    by = {c.name: c for c in em.optimizer_cases()}
    for k, own, other in (("nesterov", "plain", "reg"), ("nesterov_reg", "reg", "plain")):
        t, nt, nul = (by["%s-clip-%s" % (k, s)] for s in ("taken", "not-taken", "null"))
        for c in (t, nt):
            assert c.grad_scale != 1.0
        assert em.clip_alpha(t.alpha, t.max_gnorm, t.grad_scale, t.S, own) < t.alpha
        assert em.clip_alpha(nt.alpha, nt.max_gnorm, nt.grad_scale, nt.S, own) == nt.alpha
        assert em.clip_alpha(nt.alpha, nt.max_gnorm, nt.grad_scale, nt.S, other) < nt.alpha
        assert em.clip_alpha(t.alpha, t.max_gnorm, t.grad_scale, t.S, other) != \
            em.clip_alpha(t.alpha, t.max_gnorm, t.grad_scale, t.S, own)
        assert nul.S is None


# ---------------------------------------------------------------- liveness

def test_every_optimizer_mutation_is_noticed():
    """per kernel, every mutation that applies to it changes what at least one of its cases expects (the production
    case, 21 M elements, is left out: the small ones must do)"""
    cases = [c for c in em.optimizer_cases() if not c.production]
    seen = set()
    for kernel, muts in em.OPT_MUTATIONS.items():
        mine = sorted((c for c in cases if c.kernel == kernel), key=lambda c: c.n)
        base = {}
        for mut in muts:
            hit = None
            for c in mine:
                if mut == "first_pass_only" and c.n <= em.SS_PASS:
                    continue
                d = em.optimizer_data(c)
                if c.name not in base:
                    base[c.name] = em.optimizer_model(c, d)
                if not _same(base[c.name], em.optimizer_model(c, d, mut=mut)):
                    hit = c.name
                    break
            assert hit, "%s: no case notices %s" % (kernel, mut)
            seen.add(mut)
    assert seen == {m for ms in em.OPT_MUTATIONS.values() for m in ms}


def test_range_mutations_are_noticed_by_the_edge_cases_alone():
    """the off-by-one mutations must show on the dedicated range cases (not only by luck of a sweep)"""
    by = {c.name: c for c in em.optimizer_cases()}
    for k in ("sumsq_reg", "nesterov_reg"):
        for name in ("ranges-1", "ranges-128", "ranges-edges"):
            c = by["%s-%s" % (k, name)]
            d = em.optimizer_data(c)
            base = em.optimizer_model(c, d)
            for mut in ("range_beg_exclusive", "range_end_inclusive", "parity_inverted"):
                assert not _same(base, em.optimizer_model(c, d, mut=mut)), (c.name, mut)
        c0 = by["%s-ranges-0" % k]
        d0 = em.optimizer_data(c0)
        assert not _same(em.optimizer_model(c0, d0), em.optimizer_model(c0, d0, mut="parity_inverted"))
    e = em.edge_ranges(4099).reshape(-1, 2)
    assert e[0, 0] == 0 and e[-1, 1] == 4099 and (e[:, 0] == e[:, 1]).any() and (e[1:, 0] == e[:-1, 1]).any()
    assert (e[:, 1] - e[:, 0] == 1).any()
    assert len(em.many_ranges(4099)) == 2 * em.MAX_NOREG_RANGES


def _img(n, dtype=np.uint16):
    return np.full(n, em.SENT16 if dtype == np.uint16 else em.SENT, dtype=dtype)


def _differs(a, b):
    for k in a:
        if (a[k] is None) != (b[k] is None):
            return True
        if a[k] is not None and a[k].tobytes() != b[k].tobytes():
            return True
    return False


def test_every_launcher_mutation_is_noticed():
    seen = set()

    def note(mut, changed, what):
        assert changed, "%s: %s is not noticed" % (what, mut)
        seen.add(mut)

    # the float4 kernels, on the small sizes and one that wraps
    for n in (1028, em.F4_NS[-1]):
        a, b = em.add16_inputs(n, 7)
        i16 = {k: _img(n, np.float32 if k == "out" else np.uint16) for k in em.ADD16_OUTPUTS}
        base = em.add16(i16, a, b, n)
        for mut in ("skip_last_partial_block", "first_pass_only", "f16_truncates", "bf16_truncates", "f16_ties_away",
                    "bf16_ties_away", "add16_input_shadows_swapped"):
            if mut == "first_pass_only" and n <= em.F4_PASS:
                continue
            note(mut, _differs(base, em.add16(i16, a, b, n, mut)), "add16 n=%d" % n)
            if "shadows_swapped" not in mut:
                ic = {"f16": _img(n), "bf16": _img(n)}
                note(mut, _differs(em.cvt16(ic, a, n), em.cvt16(ic, a, n, mut)), "cvt16 n=%d" % n)
            if "16" not in mut:
                o = _img(n, np.float32)
                note(mut, em.add(o, a, b, n).tobytes() != em.add(o, a, b, n, mut).tobytes(), "add n=%d" % n)
    # each rounding mutation on its own shadow only
    n = 1028
    ic = {"f16": _img(n), "bf16": _img(n)}
    src = em.shadow_data(n, 5)
    base = em.cvt16(ic, src, n)
    for mut, k, other in (("f16_truncates", "f16", "bf16"), ("f16_ties_away", "f16", "bf16"),
                          ("bf16_truncates", "bf16", "f16"), ("bf16_ties_away", "bf16", "f16")):
        got = em.cvt16(ic, src, n, mut)
        assert not np.array_equal(got[k], base[k]) and np.array_equal(got[other], base[other]), mut
    # gathers: the padding mutations need ldd > cols (unwritten) and ldd > ceil64(cols) (64-lane round-up)
    hits = {"gather_padding_unwritten": 0, "gather_pads_to_64_lanes": 0, "bf16_truncates": 0, "f16_ties_away": 0}
    for c in em.row_cases():
        img = {"dst": _img(c.dst_elems, np.float32), "f16": _img(c.dst_elems), "bf16": _img(c.dst_elems)}
        base = em.gather_rows16(img, c.ldd, c.src, c.lds, c.idx, c.rows, c.cols)
        assert not np.isnan(base["dst"].reshape(c.rows, c.ldd)[:, c.cols:]).any(), c.name
        for mut in hits:
            hits[mut] += _differs(base, em.gather_rows16(img, c.ldd, c.src, c.lds, c.idx, c.rows, c.cols, mut))
        assert len(set(c.idx.tolist())) < c.rows or c.rows == 1, c.name                 # duplicates
    assert any((np.diff(c.idx) < 0).any() for c in em.row_cases())                      # out of order
    for mut, k in hits.items():
        note(mut, k > 0, "gather_rows16")
    assert hits["gather_padding_unwritten"] >= len(em.ROWS) * (len(em.COLS) - 1)       # every shape with padding
    for c in em.row_cases(scatter=True):
        assert sorted(set(c.idx.tolist())) == sorted(c.idx.tolist()), c.name            # a permutation: no race
    # the transpose
    hit_t = 0
    for c in em.transpose_cases():
        t0 = _img(c.cols * c.ldd)
        base = em.transpose_bf16(t0, c.ldd, c.src, c.lds, c.rows, c.cols)
        if c.rows * c.cols > 1:
            hit_t += base.tobytes() != em.transpose_bf16(t0, c.ldd, c.src, c.lds, c.rows, c.cols,
                                                         "transpose_untransposed").tobytes()
    note("transpose_untransposed", hit_t >= len(em.transpose_cases()) - 1, "transpose_bf16")
    opt = {m for ms in em.OPT_MUTATIONS.values() for m in ms}
    assert seen | opt == set(em.MUTATIONS), sorted(set(em.MUTATIONS) - seen - opt)


def test_shadow_specials_hold_what_the_table_promises():
    sp = em.shadow_specials()
    h, b = em.f16_bits(sp), em.bf16_bits(sp)
    for bits in (0x0000, 0x8000, 0x7C00, 0xFC00, 0x7BFF, 0x0001, 0x0400, 0x6800, 0x6802):
        assert bits in h.tolist(), hex(bits)
    assert np.isnan(sp).any() and em.isnan16(h, "f16").any() and em.isnan16(b, "bf16").any()
    assert (sp == np.float32(3.4028234663852886e38)).any()
    den = (np.abs(sp) > 0) & (np.abs(sp) < np.float32(2.0 ** -126))
    assert den.sum() >= 8 and set(b[den].tolist()) >= {0x0000, 0x0001, 0x0002, 0x8001}
    # every rounding mutant differs from nearest-even on the specials alone, in both directions of a tie
    for fn in (em.f16_bits, em.bf16_bits):
        for mode in ("trunc", "ties_away"):
            diff = fn(sp, mode).astype(np.int32) - fn(sp).astype(np.int32)
            assert (diff != 0).any(), (fn.__name__, mode)
        t = fn(sp, "ties_away").astype(np.int32) - fn(sp, "trunc").astype(np.int32)
        ties = t == 1
        rne = fn(sp).astype(np.int32) - fn(sp, "trunc").astype(np.int32)
        assert (rne[ties] == 0).any() and (rne[ties] == 1).any(), fn.__name__       # ties to even: both ways


# ---------------------------------------------------------------- the production layout and the rejections

def test_production_layout_is_the_engines(libs):
    """sctc_brnn_query / the tensor table need no GPU: the layout the model builds from cudamat.padded_layout is the
    one the engine reports for the cfg-3 network, bias ranges included"""
    _sctc, _ = libs
    n, ranges = em.production_layout()
    assert 20e6 < n < 23e6 and len(ranges) == 12
    cfg = _sctc.BrnnConfig(483, 33, 1824, 5, 3, 1000, 1, 20.0, 0.0, 1, _sctc.F32)
    sizes = _sctc.BrnnSizes()
    assert _sctc.lib().sctc_brnn_query(ctypes.byref(cfg), ctypes.byref(sizes)) == 0
    assert sizes.param_elems == n


def test_argument_rejections(libs):
    """checked before any launch, so no GPU is needed: no pointer is dereferenced.  Without a device the pointers are
    a made-up address; where this runs next to one they are a real, zeroed device buffer larger than anything a call
    here could touch, so that a check that stops rejecting shows as a failed assertion, never as a launch on a wild
    pointer.  (tests/test_gpu_elementwise.py repeats the rejections on guarded buffers and checks nothing is written.)"""
    _sctc, diag = libs
    L, D = _sctc.lib(), diag.lib()
    import torch
    if torch.cuda.is_available():
        backing = torch.zeros(1 << 14, dtype=torch.float32, device="cuda")     # 64 KiB: n <= 1026 floats, 8 KiB workspace
        torch.cuda.synchronize()
        P = backing.data_ptr()
    else:
        P = 0x10000

    def err():
        return L.sctc_last_error().decode()

    for name, k, flat in em.BAD_RANGES:
        arr = None if flat is None else _sctc.i64(flat)
        rc = L.sctc_nesterov_step_reg(P, P, P, 1000, 0.5, 0.125, 128.0, 0.25, 0.25, arr, k, None, None)
        assert rc == -1 and "noreg ranges" in err(), (name, rc, err())
        rc = L.sctc_sumsq_reg(P, P, P, 0.5, 0.25, 0.25, 1000, arr, k, P, P, 8192, None)
        assert rc == -1 and "noreg ranges" in err(), (name, rc, err())
    assert L.sctc_sumsq(P, 1000, P, P, 8191, None) == -3 and "workspace" in err()
    assert L.sctc_sumsq_reg(P, P, P, 0.5, 0.25, 0.25, 1000, None, 0, P, P, 8191, None) == -3 and "workspace" in err()
    for n in (1, 2, 3, 1026):
        assert D.sctc_diag_add(P, P, P, n, None) == -1 and "multiple of 4" in err()
        assert D.sctc_diag_cvt16(P, P, P, n, None) == -1 and "multiple of 4" in err()
        assert D.sctc_diag_add16(P, P, P, P, P, P, P, n, None) == -1 and "multiple of 4" in err()
    # nothing to do: rc 0 without a launch
    assert L.sctc_axpy(P, P, 1.0, 0, None) == 0 and L.sctc_scale(P, 1.0, 0, None) == 0
    assert L.sctc_nesterov_step(P, P, P, 0, 0.5, 0.1, 1.0, 1.0, None, None) == 0
    assert L.sctc_nesterov_step_reg(P, P, P, 0, 0.5, 0.1, 1.0, 1.0, 0.1, None, 0, None, None) == 0
    assert D.sctc_diag_cvt16(P, None, None, 1024, None) == 0
    assert D.sctc_diag_add(P, P, P, 0, None) == 0 and D.sctc_diag_gather_rows(P, 64, P, 3, P, 0, 3, None) == 0
