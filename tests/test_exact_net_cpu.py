"""tests/exact_net.py is right, and the comparison the GPU suite makes with it has teeth (CPU only).

* the batched reference equals oracle.brnn utterance by utterance: everything the forward pass computes BIT for bit
  (the arithmetic is exact, so the batching cannot change a bit), the backward pass to 1e-12 relative;
* make_case's conditions (integers below 2^22, the shares of open / zero / clipped units, pre-activations exactly on
  both boundaries, every 16 x 16 block of Wf / Wb occupied, no skip) hold for every entry of the GPU matrix;
* mutants of the reference itself -- a dropped K chunk of one row block, a stale state, a backward direction started
  at the wrong frame, swapped rows, a non-strict mask, a ceiling off by 2^-20 -- are all reported by the very
  comparison tests/test_gpu_recurrence_exact.py applies to the device's buffers;
* the rounding model of the fp16-operand backward pass (exact_net.Rounding) changes nothing when it is off, equals
  oracle.brnn.Mixed utterance by utterance when it accumulates in float64, keeps its own float32 noise within what the
  GPU suite's bounds assume on every f16 row of the matrix, and every wrong rounding point -- truncation, a recurrence
  that rounds when it should not or the reverse, a 16-bit BPTT state, bias gradients of unrounded deltas, a dropped
  BPTT step, float16 delta shadows, one unrounded GEMM operand, row pairs one frame late -- breaks one of those bounds."""
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


def _sum_grads(a, b):
    return b if a is None else {"W": [x + y for x, y in zip(a["W"], b["W"])], "b": [x + y for x, y in zip(a["b"], b["b"])],
                                "Wf": a["Wf"] + b["Wf"], "Wb": a["Wb"] + b["Wb"]}


@pytest.mark.parametrize("H,B", [(96, 5), (512, 6)])
def test_mixed_none_is_the_reference_of_before(H, B):
    """the rounding model is an option: without it the same operations run on the same arrays, so the result is the
    same bit for bit in both accumulation types (the identity stands where a rounding would) -- and it still equals the
    unrounded oracle (test_reference_equals_oracle)"""
    case = en.make_case(H, B)
    for dt in (np.float64, np.float32):
        a, b = en.reference(case, dt), en.reference(case, dt, mixed=None)
        for (name, x), (_, y) in zip(en.grad_tensors(a["grads"]), en.grad_tensors(b["grads"])):
            assert x.dtype == dt and y.dtype == dt
            _same(x, y)
        for k in ("d1", "dF", "dB"):
            for x, y in zip(a[k], b[k]):
                _same(x, y)
        assert "shadows" not in a
    # dF + dB is the delta entering the temporal layer's weight gradient: with TL = 1 that is d1
    assert case.TL == 1
    for d1, dF, dB in zip(a["d1"], a["dF"], a["dB"]):
        _same(d1, dF + dB)


@pytest.mark.parametrize("H,B", [(96, 5), (512, 6)])
@pytest.mark.parametrize("rec", [True, False])
def test_rounding_model_equals_oracle_mixed(H, B, rec):
    """float64 accumulation: the batched rounding model is oracle.brnn's Mixed, utterance by utterance"""
    case = en.make_case(H, B)
    m64 = en.reference(case, mixed=en.Rounding(rec))
    total = None
    for b in range(B):
        out = {}
        c, g, s, _ = obrnn.cost_and_grad(case.params, case.datas[b], case.labs[b], case.TL, max_act=case.max_act,
                                         mixed=obrnn.Mixed(rec=rec), cache_out=out)
        assert not s and m64["costs"][b] == pytest.approx(c, rel=1e-12)        # the forward pass is exact either way
        _same(m64["hF"][b], out["hF"])
        _same(m64["hB"][b], out["hB"])
        assert en.rel_fro(m64["d1"][b], out["d1"]) <= 1e-12
        _same(m64["shadows"]["d1"][b], obrnn.round_bf16(m64["d1"][b]))
        total = _sum_grads(total, g)
    for (name, got), (_, want) in zip(en.grad_tensors(m64["grads"]), en.grad_tensors(total)):
        assert en.rel_fro(got, want) <= 1e-12, name
    # and it is not the unrounded reference: bfloat16 operands cost 1e-4 .. 5e-2 per tensor
    ex = en.reference(case)
    for (name, got), (_, want) in zip(en.grad_tensors(m64["grads"]), en.grad_tensors(ex["grads"])):
        assert 1e-4 < en.rel_fro(got, want) < 5e-2, name


def _f16_rows():
    seen, rows = set(), []
    for c in en.GPU_CASES:
        key = (c.H, c.B, c.NL, c.TL, c.Tmax, c.path == "mh")
        if c.mode == "f16" and key not in seen:
            seen.add(key)
            rows.append(c)
    return rows


@pytest.mark.parametrize("c", _f16_rows(), ids=lambda c: c.id)
def test_rounding_model_conditions_on_the_f16_rows(c):
    """what the GPU suite's bounds rest on, on the models alone: the float32-accumulating model differs from the float64
    one (else 16 x e_ref would be the floor everywhere and the seeds pointless) wherever a sum is long or passes
    through the recurrence -- dW1, dWf, dWb, deltasFor, deltasBack; the gradients above the temporal layer are sums of a
    few hundred bfloat16 values of similar size, which fp32 may well add without any error, so 0 is allowed there and the
    floor of 2^-24 holds the device -- and its bfloat16 shadows differ from the float64 model's in at most 2e-4 of their
    elements, a fifth of what the device is allowed, on each of the eight seeds.  One flipped element of delta_1's shadow
    is 2^-8 of itself and can be 4e-4 of dW1 (16 features: mh-H1024-B12, seed 2), so e_ref is not small everywhere; what
    it must stay below is 5e-2 / 16, or the model's bound would be looser than the configuration's own 5e-2."""
    assert 12 <= c.Tmax <= 16
    e_ref = en.mixed_e_ref(c.H, c.B, c.NL, c.TL, c.Tmax, c.path == "mh")
    for k in ("fro:dW1", "fro:dWf", "fro:dWb", "row:dF", "row:dB"):
        assert e_ref[k] > 0, k
    for k, v in e_ref.items():
        kind = k.split(":")[0]
        if kind == "share":
            assert v <= en.REF_SHADOW_SHARE, (k, v)
        elif kind in ("open", "dirty"):
            assert v == 0, (k, v)
        else:
            assert v < 5e-2 / 16, (k, v)
    assert en.rounding_of(c) == en.Rounding(c.path == "mh")


def backward_mutants(case):
    """(name, argument) of every backward mutant of the rounding model for this case"""
    pl, NL, TL = case.plan, case.NL, case.TL
    short = min((b for b in range(pl.B) if case.Ts[b] > 1), key=lambda b: (case.Ts[b], b))
    out = [("trunc", None), ("rec_flip", None), ("state16", None), ("db_unrounded", None), ("f16_shadow", None),
           ("pair_shift", short)]
    out += [("drop_bptt", u) for u in (0, pl.Tmax // 2, pl.Tmax - 2)]
    # one operand of one GEMM unrounded: the A (delta) operand of every kind of GEMM.  The B operands are left out,
    # because on these networks they are no mutants: every value of the +-1 / power-of-two weights, the features, hF, hB
    # and their sum is a bfloat16 value already (asserted); a ReLU layer's output is one unless it has an odd value
    # above 256 (then its rounding is a mutant, and in the list)
    for m in case.params["W"] + [case.params["Wf"], case.params["Wb"], case.fwd["acts"][0], case.fwd["acts"][TL],
                                 case.fwd["hF"], case.fwd["hB"]]:
        assert np.array_equal(obrnn.round_bf16(m), m)
    out += [("unrounded", w) for w in [("dW", NL, "A"), ("dgrad", NL, "A"), ("dW", TL, "A"), ("dgrad", TL, "A"),
                                       ("dW", 0, "A"), ("dWf", "A"), ("dWb", "A")]]
    out += [("unrounded", ("dW", i, "B")) for i in range(1, NL + 1)
            if not np.array_equal(obrnn.round_bf16(case.fwd["acts"][i]), case.fwd["acts"][i])]
    return out


@pytest.mark.parametrize("H,B,rec", [(512, 6, True), (512, 24, False), (96, 5, False)])
def test_backward_comparison_reports_every_rounding_mutant(H, B, rec):
    """every wrong rounding point, run with float32 accumulation like a device would, breaks one of the GPU suite's rules
    at the GPU suite's bounds (exact_net.mixed_violations: per tensor and per frame 16 x e_ref, shadow shares 1e-3, zeros)
    -- for a 16-bit-exchange shape, a fp32-recurrence shape and the generic layer size; the float32 model itself breaks
    none.  A mutant no statistic sees is a failure of the statistics."""
    case = en.make_case(H, B)
    mixed = en.Rounding(rec)
    e_ref = en.mixed_e_ref(H, B, case.NL, case.TL, case.dims[5], rec)
    m64 = en.reference(case, mixed=mixed)
    verdict = lambda mutant: en.mixed_violations(en.mixed_stats(en.reference(case, np.float32, mixed=mixed, mutant=mutant),
                                                                m64, case.max_act), e_ref, 16.0)
    assert verdict(None) == []
    missed = [m for m in backward_mutants(case) if not verdict(m)]
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
