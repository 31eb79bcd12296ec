"""CPU-side half of the direct GEMM option tests (tests/test_gpu_gemm_options.py): the float64 model of GemmArgs
(tests/gemm_model.py) against hand-computed cases; the precondition that makes the GPU comparison BIT-exact, for
every case of the table (tests/gemm_cases.py); liveness -- every case notices every mutation of the model that applies
to it, so a kernel with that mistake cannot pass; the argument rejections of launch_gemm_f32, which need no GPU; and
the ctypes mirror of sctc_diag_gemm_args against the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import gemm_cases as gc
from tests import gemm_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    import _sctc
    from tools.diag import sctc_diag
    if not (os.path.exists(_sctc.LIB_PATH) and os.path.exists(sctc_diag.LIB_PATH)):
        ge.build()
    return _sctc.lib(), sctc_diag


# ---------------------------------------------------------------- the model, by hand

def test_model_epilogue_order_by_hand():
    """acc = A (B is the identity); + bias -> relu -> mask -> + 0.25 addend -> + C_prev"""
    g = gm.args(A=[[1, 2, NAN], [3, 4, NAN]], B=[[1, 0], [0, 1]], M=2, N=2, K=2, bias=[-2, 1], relu=1,
                mask=np.array([[2.0, -0.0, NAN], [1e-45, 0.0, NAN]], dtype=np.float32),
                addend=[[4, 8], [-4, 0]], add_scale=0.25, accumulate=1, C=[[10, 20, -7], [30, 40, -7]])
    out = gm.gemm_model(g)
    #   acc + bias      relu            mask (> 0: 2.0 and the denormal)   + addend / 4     + C_prev
    # [[-1, 3], [1, 5]] [[0, 3], [1, 5]] [[0, 0], [1, 0]]                  [[1, 2], [0, 0]] [[11, 22], [30, 40]]   (addend / 4 = [[1, 2], [-1, 0]])
    assert out.C.tolist() == [[11, 22], [30, 40]]
    assert out.C16a is None and out.C16b is None and out.colsum_a is None and out.a_sum is None
    assert gm.gemm_model(g, "mask_last").C.tolist() == [[11, 20], [30, 40]]
    assert gm.gemm_model(g, "mask_first").C.tolist() == [[11, 23], [30, 41]]
    assert gm.gemm_model(g, "mask_negzero_positive").C.tolist() == [[11, 25], [30, 40]]


def test_model_gather_and_column_sums_by_hand():
    """row-contiguous operands with K-row gathers: A(m,k) = A[idx_a[k]][m]; no index names row 1 of A or of B"""
    g = gm.args(A=[[1, 2, NAN], [NAN, NAN, NAN], [3, 4, NAN]], idx_a=[2, 0, 2], a_kcontig=0,
                B=[[1, NAN], [NAN, NAN], [100, NAN], [NAN, NAN]], idx_b=[0, 0, 2], b_kcontig=0, M=2, N=1, K=3,
                accumulate=1, C=[[1], [2]], colsum_a=[1, 1, -7])
    out = gm.gemm_model(g)
    assert out.C.tolist() == [[3 + 1 + 300 + 1], [4 + 2 + 400 + 2]]
    assert out.colsum_a.tolist() == [3 + 1 + 3 + 1, 4 + 2 + 4 + 1]
    assert gm.gemm_model(g, "swap_idx").C.tolist() == [[100 + 1 + 300 + 1], [200 + 2 + 400 + 2]]
    assert gm.gemm_model(g, "drop_last_k").colsum_a.tolist() == [5, 7]


def test_model_two_addend_operand_by_hand():
    g = gm.args(A=[[1, 2, NAN]], A2=[[10, 20, NAN]], B=[[1, 1]], M=1, N=1, K=2, a_sum=True, colsum_a=[0.0])
    out = gm.gemm_model(g)
    assert out.C.tolist() == [[33]] and out.a_sum.tolist() == [[11, 22]]
    assert out.colsum_a is None                                   # K-contiguous A: untouched
    assert gm.gemm_model(g, "a2_not_in_product").C.tolist() == [[3]]


def test_model_shadows_by_hand():
    """16-bit operands in memory, 16-bit mask, both shadows, no fp32 result: 2049 and 2051 are ties in float16
    (spacing 2 above 2048: to even, 2048 and 2052) and round down to 2048 in bfloat16 (spacing 16)"""
    g = gm.args(A=[[1]], B=[[1], [1], [1]], M=1, N=3, K=1, prec=1, in16=1, bias=[2048, 2050, 5],
                mask16=np.array([[0x0001, 0x3C00, 0x8000]], dtype=np.uint16), C16a=True, C16b=True, skip_c32=1)
    out = gm.gemm_model(g)
    assert out.C is None
    assert out.C16a.tolist() == [[0x6800, 0x6802, 0x0000]]
    assert out.C16b.tolist() == [[0x4500, 0x4500, 0x0000]]
    assert gm.gemm_model(g, "shadow_round_to_zero").C16a.tolist() == [[0x6800, 0x6801, 0x0000]]
    assert gm.gemm_model(g, "write_c_despite_skip").C.tolist() == [[2049, 2051, 0]]


# ---------------------------------------------------------------- the GPU table: exactness and liveness

def planned_splits(diag, monkeypatch, c):
    """the split-K count of case c: its own, or the planner's (a host function: no GPU needed)"""
    if "planner" not in c.opts:
        return c.splits
    im = gc.IMPLS[c.impl]
    for n in gc.ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    for n, v in im["env"].items():
        monkeypatch.setenv(n, v)
    return diag.gemm_plan(c.M, c.N, c.K, c.lay, im["prec"], im["in16"], "gather" in c.opts, "a2" in c.opts).splits


@pytest.mark.parametrize("impl", sorted(gc.IMPLS))
def test_cases_are_exact_in_fp32(impl):
    """operands representable in the operand type; every value the epilogue can form is a multiple of 2^-2 below
    2^21 (so every fp32 summation order is exact) and below 65504 (float16 shadows cannot overflow)"""
    im = gc.IMPLS[impl]
    for c in gc.cases_for(impl):
        d = gc.host_data(c)
        g = gc.model_args(c, d, splits=1)
        A = gm._logical(d.A, d.akc, d.idx_a, c.M, c.K).astype(np.float64)
        B = gm._logical(d.B, d.bkc, d.idx_b, c.N, c.K).astype(np.float64)
        parts = [A, B]
        if d.A2 is not None:
            A2 = gm._logical(d.A2, d.akc, d.idx_a, c.M, c.K).astype(np.float64)
            parts.append(A2)
            A = A + A2
        for x in parts + [A]:
            assert np.isfinite(x).all() and (x == np.round(x)).all(), c.name
            if im["prec"] in (1, 2):
                assert (gm.round_f16(x) == x).all() and (gm.round_bf16(x) == x).all(), c.name
        bound = np.abs(A) @ np.abs(B).T
        quarter = []
        if g.bias is not None:
            bound = bound + np.abs(g.bias.astype(np.float64))[None, :]
            quarter.append(g.bias)
        if g.addend is not None:
            t = gc.ADD_SCALE * d.addend[:c.M, :c.N].astype(np.float64)
            bound = bound + np.abs(t)
            quarter.append(t)
        if g.accumulate:
            bound = bound + np.abs(d.C0[:c.M, :c.N].astype(np.float64))
            quarter.append(d.C0[:c.M, :c.N])
            if d.colsum0 is not None:
                quarter.append(d.colsum0[:c.M])
        for q in quarter:
            q = np.asarray(q, dtype=np.float64)
            assert np.isfinite(q).all() and (4 * q == np.round(4 * q)).all(), c.name
        assert bound.max() < min(2.0 ** 21, 65504.0), (c.name, bound.max())
        # the column sums: integers below 2^21 as well
        assert np.abs(A).sum(axis=1).max(initial=0.0) + 8 < 2.0 ** 21, c.name


def _differs(a, b):
    for f in ("C", "C16a", "C16b", "colsum_a", "a_sum"):
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None):
            return True
        if x is not None and not np.array_equal(np.asarray(x), np.asarray(y)):    # NaN ("never stored") differs
            return True
    return False


@pytest.mark.parametrize("impl", sorted(gc.IMPLS))
def test_every_case_sees_every_mutation(impl, libs, monkeypatch):
    _, diag = libs
    used = set()
    for c in gc.cases_for(impl):
        s = planned_splits(diag, monkeypatch, c)
        d = gc.host_data(c)
        g = gc.model_args(c, d, splits=s)
        tile = gc.case_tile(c)
        base = gm.gemm_model(g, None, tile)
        for mut in gc.applicable_mutations(c, splits=s):
            assert _differs(base, gm.gemm_model(g, mut, tile)), "%s cannot see %s" % (c.name, mut)
            used.add(mut)
    im = gc.IMPLS[impl]
    want = set(gm.MUTATIONS)
    if im["prec"] != 0:
        want -= {"a2_not_in_product", "a2_not_in_asum", "asum_first_tile_rows_only"}          # A2 is prec 0 only
    if im["prec"] not in (1, 2):
        want -= {"shadow_round_to_zero", "write_c_despite_skip"}                               # no shadows
    assert used == want, "mutations no case of %s exercises: %s" % (impl, sorted(want - used))


def test_planner_can_leave_the_last_slice_empty(libs, monkeypatch):
    """fp32 kernel, 128 x 128 tiles, 76 output tiles, K = 1296 = 81 K tiles of 16: 10 slices of 9 tiles, the
    last one starts at tile 81"""
    _, diag = libs
    monkeypatch.setenv("SCTC_GEMM_SHAPE", "0")
    p = diag.gemm_plan(19 * 128, 4 * 128, 1296, "TN", 0, 0)
    assert p.splits == 10 and p.ws_floats == 10 * 19 * 128 * (4 * 128 + 1)
    per = (81 + p.splits - 1) // p.splits
    assert (p.splits - 1) * per >= 81


# ---------------------------------------------------------------- rejections (no GPU: checked before any launch)

def test_illegal_combinations_are_rejected(libs):
    L, diag = libs
    D = diag.lib()
    P = 0x10000          # a 16-byte aligned address that is never dereferenced: every call fails its argument check

    def call(**kw):
        a = diag.GemmArgs(A=P, B=P, C=P, lda=8, ldb=8, ldc=8, M=4, N=4, K=8, a_kcontig=1, b_kcontig=1, splits=1)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = D.sctc_diag_gemm(ctypes.byref(a), None)
        return rc, L.sctc_last_error().decode()

    for kw, msg in (
            (dict(C16a=P, ldc16=8, prec=0), "16-bit shadow outputs need prec != 0"),
            (dict(C16b=P, ldc16=8, prec=0), "16-bit shadow outputs need prec != 0"),
            (dict(prec=1, C16a=P, ldc16=8, skip_c32=1, accumulate=1), "skip_c32 needs"),
            (dict(prec=1, skip_c32=1), "skip_c32 needs"),
            (dict(prec=1, mask16=P, ldmask16=8, mask=P, ldmask=8), "mask16 excludes mask"),
            (dict(A2=P, a_kcontig=0, b_kcontig=0, idx_a=P), "two-addend A operand"),
            (dict(A2=P, a_kcontig=1, b_kcontig=0), "two-addend A operand"),
            (dict(A2=P, prec=3), "two-addend A operand"),
            (dict(a_sum=P), "a_sum without A2"),
            (dict(splits=2), "split-K without workspace"),
            (dict(K=-1), "negative K"),
            (dict(prec=1, in16=1, K=4), "16-bit operands need"),
    ):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert D.sctc_diag_gemm(None, None) == -1 and "null" in L.sctc_last_error().decode()


def test_diag_gemm_struct_mirror_matches_the_header(libs, tmp_path):
    """compile a tiny C program against tools/diag/sctc_diag.h and compare sizeof / offsetof with the ctypes mirror"""
    _, diag = libs
    fields = ["ldc", "K", "idx_a", "ldmask", "add_scale", "colsum_a", "splits", "in16", "C16a", "ldc16", "skip_c32",
              "mask16", "ldmask16", "A2", "a_sum"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc_diag.h"\n'
                    'int main(void){printf("%zu", sizeof(sctc_diag_gemm_args));\n' +
                    "".join('printf(" %%zu", offsetof(sctc_diag_gemm_args, %s));\n' % f for f in fields) +
                    'printf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "tools", "diag"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(diag.GemmArgs)] + [getattr(diag.GemmArgs, f).offset for f in fields]
    assert got == want
