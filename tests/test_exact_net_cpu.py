"""tests/exact_net.py is right, and the comparison the GPU suite makes with it has teeth (CPU only).

* the batched reference equals oracle.brnn utterance by utterance: everything the forward pass computes BIT for bit
  (the arithmetic is exact, so the batching cannot change a bit), the backward pass to 1e-12 relative;
* make_case's conditions (integers below 2^22, the shares of open / zero / clipped units, pre-activations exactly on
  both boundaries, every 16 x 16 block of Wf / Wb occupied, no skip) hold for every entry of the GPU matrix;
* mutants of the reference itself -- a dropped K chunk of one row block, a stale state, a backward direction started
  at the wrong frame, swapped rows, a non-strict mask, a ceiling off by 2^-20 -- are all reported by the very
  comparison tests/test_gpu_recurrence_exact.py applies to the device's buffers."""
import numpy as np
import pytest

from oracle import brnn as obrnn
from tests import exact_net as en


def _same(a, b):
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("H,B", [(96, 5), (512, 3)])
def test_reference_equals_oracle(H, B):
    case = en.make_case(H, B)
    NL, TL = case.NL, case.TL
    assert len(set(case.Ts)) > 1
    ref = en.reference(case)
    total = None
    for b in range(B):
        logits, cache = obrnn.forward(case.params, case.datas[b], TL, max_act=case.max_act)
        _same(ref["z"][b], cache["pre"][TL])
        _same(ref["preF"][b], cache["preF"])
        _same(ref["preB"][b], cache["preB"])
        _same(ref["hF"][b], cache["hF"])
        _same(ref["hB"][b], cache["hB"])
        for i in range(NL + 2):
            _same(ref["acts"][i][b], cache["acts"][i])
        _same(ref["logits"][b], logits)
        out = {}
        c, g, s, _ = obrnn.cost_and_grad(case.params, case.datas[b], case.labs[b], TL, max_act=case.max_act, cache_out=out)
        assert not s and not ref["skips"][b]
        assert ref["costs"][b] == pytest.approx(c, rel=1e-12)
        assert en.rel_fro(ref["d1"][b], out["d1"]) <= 1e-12
        if total is None:
            total = g
        else:
            total = {"W": [x + y for x, y in zip(total["W"], g["W"])], "b": [x + y for x, y in zip(total["b"], g["b"])],
                     "Wf": total["Wf"] + g["Wf"], "Wb": total["Wb"] + g["Wb"]}
    for (name, got), (_, want) in zip(en.grad_tensors(ref["grads"]), en.grad_tensors(total)):
        assert en.rel_fro(got, want) <= 1e-12, name


def test_float32_backward_is_close_but_not_equal():
    """the dtype switch really runs the backward part in float32: its per-frame error against float64 is that of
    fp32 arithmetic -- not zero, and far below the 1e-4 bar the device is held to"""
    case = en.make_case(96, 5)
    r64, r32 = en.reference(case), en.reference(case, dtype=np.float32)
    assert r32["d1"][0].dtype == np.float32 and r32["grads"]["Wf"].dtype == np.float32
    rho, dirty = en.row_errors(r32["d1"], r64["d1"])
    assert dirty == 0 and 0 < rho < 1e-5, rho
    assert en.forward_rows_differing(r32, r64) == 0


def test_conditions_hold_for_the_gpu_matrix():
    """make_case asserts them; here for every (H, B, NL, TL, Tmax, seed) the GPU suite uses.  Also: the matrix covers
    what it is meant to cover -- every length rule of make_case, and unsorted caller orders"""
    seen = set()
    for c in en.GPU_CASES:
        key = (c.H, c.B, c.NL, c.TL, c.Tmax, c.seed)
        if key in seen:
            continue
        seen.add(key)
        case = en.gpu_case(c)
        assert 12 <= c.Tmax <= 16 and max(case.Ts) == c.Tmax and len(case.Ts) == c.B
        if c.B >= 3:
            assert case.Ts.count(1) >= 1 and case.Ts.count(c.Tmax) >= 2
            assert case.Ts != sorted(case.Ts, reverse=True)
        for d in ("F", "B"):
            s = case.stats[d]
            assert s["open"] >= 0.05 and s["zero"] >= 0.10 and s["clipped"] >= 0.10
    assert len({c.id for c in en.GPU_CASES}) == len(en.GPU_CASES)


def _mutants(case):
    """(name, argument) of every forward mutant for this case"""
    H = case.dims[2]
    pl = case.plan
    rs = np.random.RandomState(H)
    if H <= 96:         # small layer: every (16-row block, 32-column chunk)
        chunks = [(r, c) for r in range(0, H, 16) for c in range(0, H, 32)]
    else:
        chunks = [(16 * int(rs.randint(H // 16)), 32 * int(rs.randint(H // 32))) for _ in range(6)] + [(H - 16, H - 32), (0, 0)]
    out = [("drop_wf", rc) for rc in chunks] + [("drop_wb", rc) for rc in chunks]
    out += [("stale_h", t) for t in (2, pl.Tmax // 2, pl.Tmax - 1)]
    short = [b for b in range(pl.B) if 1 < case.Ts[b] < pl.Tmax]
    out += [("back_start", b) for b in short[:2]] + [("back_start", case.Ts.index(1))]
    longest = [b for b in range(pl.B) if case.Ts[b] == pl.Tmax]
    out += [("swap_rows", (longest[0], longest[1]))]
    out += [("max_act", case.max_act - 2.0 ** -20)]
    return out


@pytest.mark.parametrize("H,B", [(96, 5), (512, 6)])
def test_forward_comparison_reports_every_mutant(H, B):
    case = en.make_case(H, B)
    ref = en.reference(case, backward=False)
    assert en.forward_rows_differing(ref, ref) == 0
    missed = []
    for mutant in _mutants(case):
        got = en.reference(case, backward=False, mutant=mutant)
        n_rows = en.forward_rows_differing(got, ref, names=("hF", "hB"))
        differs = any(not np.array_equal(np.float32(g), np.float32(r))
                      for n in ("hF", "hB") for g, r in zip(got[n], ref[n]))
        assert differs == (n_rows > 0)
        if n_rows == 0:
            missed.append(mutant)
    assert not missed, missed


def test_backward_comparison_reports_a_nonstrict_mask():
    """h >= 0, h <= maxAct instead of 0 < h < maxAct: with hundreds of units exactly on either boundary and most of
    the others clipped, delta_1 moves by far more than the backward tolerance of the GPU suite (1e-4 per frame)"""
    case = en.make_case(96, 5)
    ref = en.reference(case)
    got = en.reference(case, mutant=("nonstrict_mask", None))
    assert en.forward_rows_differing(got, ref) == 0           # a backward-only mutant
    rho, _ = en.row_errors(got["d1"], ref["d1"])
    assert rho > 1e-4, rho
    rho32, _ = en.row_errors(en.reference(case, dtype=np.float32)["d1"], ref["d1"])
    assert rho > 16 * rho32
    assert max(en.rel_fro(g, w) for (_, g), (_, w) in zip(en.grad_tensors(got["grads"]), en.grad_tensors(ref["grads"]))) > 1e-4
