"""sctc_nbest_mbr_batch on the GPU against tests/mbr_model.py.

  * the distances: bit-equal to edit_model for K = 1, 2, 3, 40, 256, one and several panels, ragged and empty
    hypotheses, K_b < K, -inf and NaN scores inside K_b, both units; symmetric, zero diagonal;
  * equal scores: every weight is exactly 1.0 and every sum an integer, so posteriors, risks, choice, order and
    confidences are bit-equal to the model, constructed ties included;
  * general scores: posteriors, risks and confidences within relative 1e-12.  float64 exp() on the device and in libm
    may differ by a few ulp (2.2e-16) and at most 256 products are added: 256 x 4 ulp is about 2e-13, the bound leaves
    a factor of five.  `best`, `order` and the confidences are compared on the seeds whose neighbouring model risks
    differ by more than 1e-9 relative (at scale 0, where all is exact, on every seed); at most one seed in ten of a
    scale's list may be set aside, and that is asserted at each of the scales 0, 1 and 50;
  * confidences; the composition with the search and the second pass in place on their tensors.
Whole output buffers are compared, each with guard words behind it, and the workspace is exactly the size asked for."""
import ctypes
import math

import numpy as np
import pytest

from tests import beam_trace as bt
from tests import mbr_model as M

pytestmark = pytest.mark.gpu

SP = 1
TAIL = 8
GI = -0x21524111          # guard of the int32 buffers
GD = -1.25e300            # and of the float64 ones
CONF, DIST = 1, 2


def bounds(hyps, K_b, unit):
    B, K = len(hyps), len(hyps[0])
    b = np.array([[((len(h) + 1) // 2 if unit == "word" else len(h)) if k < K_b[i] else 0 for k, h in enumerate(row)]
                  for i, row in enumerate(hyps)], dtype=np.int64).reshape(B, K)
    return np.concatenate([[0], np.cumsum(b.max(axis=1))]).astype(np.int64)


def run_mbr(hyps, scores, unit="char", scale=1.0, A=8, order=None, K_b=None, conf=False):
    """the raw entry with SCTC_MBR_DIST; returns the whole buffers, guards included, and the confidence offsets"""
    import torch
    import _sctc
    B, K = len(hyps), len(hyps[0])
    rows = [np.asarray(h, dtype=np.int32).reshape(-1) for row in hyps for h in row]
    U = np.array([len(r) for r in rows], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(U)[:-1]]).astype(np.int64)
    labels = torch.from_numpy(np.concatenate(rows + [np.zeros(1, np.int32)])).cuda()
    Kb = np.full(B, K, dtype=np.int32) if K_b is None else np.asarray(K_b, dtype=np.int32)
    flags = DIST | (CONF if conf else 0)
    cfg = _sctc.MbrConfig(B, K, 1 if unit == "word" else 0, flags, A, SP, float(scale), _sctc.i32(Kb), _sctc.i32(U), _sctc.i64(off))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_nbest_mbr_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), "test")
    sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)).cuda()
    od = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32).reshape(-1)).cuda()
    first = bounds(hyps, Kb, unit)

    def buf(n, dtype, fill):
        return torch.full((n + TAIL,), fill, dtype=dtype, device="cuda")
    out = {"posterior": buf(B * K, torch.float64, GD), "risk": buf(B * K, torch.float64, GD), "best": buf(B, torch.int32, GI),
           "order": buf(B * K, torch.int32, GI), "dist": buf(B * K * K, torch.int32, GI),
           "confidence": buf(int(first[-1]), torch.float64, GD), "conf_len": buf(B, torch.int32, GI)}
    ws = torch.full((nbytes.value + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.sctc_nbest_mbr_batch(ctypes.byref(cfg), labels.data_ptr(), sc.data_ptr(), od.data_ptr() if od is not None else None,
                                out["posterior"].data_ptr(), out["risk"].data_ptr(), out["best"].data_ptr(),
                                out["order"].data_ptr(), out["dist"].data_ptr(),
                                out["confidence"].data_ptr() if conf else None, out["conf_len"].data_ptr() if conf else None,
                                ws.data_ptr(), nbytes.value, _sctc.current_stream_ptr())
    _sctc.check(rc, "test")
    assert (ws[nbytes.value:].cpu().numpy() == 0xA5).all(), "the call wrote behind its workspace"
    return {k: v.cpu().numpy() for k, v in out.items()}, first


def want_buffers(hyps, scores, first, unit="char", scale=1.0, A=8, order=None, K_b=None, conf=False):
    r = M.mbr(hyps, scores, unit=unit, scale=scale, space=SP, A=A, order=order, K_b=K_b, confidences=True)
    ti, td = np.full(TAIL, GI, dtype=np.int32), np.full(TAIL, GD)
    flat = np.full(int(first[-1]), GD)
    clen = np.full(len(hyps), GI, dtype=np.int32)
    if conf:
        clen = r["conf_len"]
        for b, c in enumerate(r["confidence"]):
            flat[first[b]:first[b] + len(c)] = c
    return {"posterior": np.concatenate([r["posterior"].reshape(-1), td]), "risk": np.concatenate([r["risk"].reshape(-1), td]),
            "best": np.concatenate([r["best"], ti]), "order": np.concatenate([r["order"].reshape(-1), ti]),
            "dist": np.concatenate([r["dist"].reshape(-1), ti]), "confidence": np.concatenate([flat, td]),
            "conf_len": np.concatenate([clen, ti])}, r


def same_bits(got, want, keys=None):
    for k in keys or want:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), "%s differs: %s" % (k, np.nonzero(g != w)[0][:8])


def random_lists(seed, B, K, max_len, alphabet=6, distinct=False):
    """rows over symbols 1..alphabet-1 (1 is the space); two hypotheses in three are edits of the one before.
    distinct: no hypothesis twice in an utterance, neither as symbols nor as words (equal hypotheses have equal
    risks)"""
    rs = np.random.RandomState(seed)
    hyps = []
    for _ in range(B):
        row = [rs.randint(1, alphabet, size=int(rs.randint(0, max_len + 1))).astype(np.int32)]
        seen = {tuple(row[0]), tuple(M.tokens(row[0], SP))}
        while len(row) < K:
            k = len(row)
            h = list(row[-1]) if k % 3 else list(rs.randint(1, alphabet, size=int(rs.randint(0, max_len + 1))))
            for _ in range(int(rs.randint(0, 4))):
                pos = int(rs.randint(0, len(h) + 1))
                if rs.rand() < 0.5 or not h:
                    h.insert(pos, int(rs.randint(1, alphabet)))
                else:
                    del h[min(pos, len(h) - 1)]
            h = h[:max_len]
            if distinct and (tuple(h) in seen or tuple(M.tokens(h, SP)) in seen):
                continue
            seen.update((tuple(h), tuple(M.tokens(h, SP))))
            row.append(np.array(h, dtype=np.int32))
        hyps.append(row)
    return hyps, rs


# ---- 1. the distances, and everything else in the exact case ----------------------------------------------------------

@pytest.mark.parametrize("unit", ["char", "word"])
@pytest.mark.parametrize("K,B,max_len", [(1, 3, 20), (2, 5, 30), (3, 5, 30), (40, 2, 24), (256, 1, 4)])
def test_equal_scores_bit_equal(unit, K, B, max_len):
    """equal scores among the real ranks, some ranks not real (K_b < K, -inf, NaN, +inf): every buffer bit for bit"""
    hyps, rs = random_lists(100 + K, B, K, max_len, alphabet=4 if K == 256 else 6)
    hyps[0][0] = np.zeros(0, np.int32)                          # an empty hypothesis among the real ones
    K_b = [K] + [int(rs.randint(0, K + 1)) for _ in range(B - 1)]
    scores = np.full((B, K), -12.5)
    for b in range(B):
        for k in range(2, K, 5):
            scores[b, k] = (-math.inf, math.nan, math.inf)[(b + k) % 3]
    order = np.array([rs.permutation(K) for _ in range(B)], dtype=np.int32)
    for od in (None, order):
        got, first = run_mbr(hyps, scores, unit=unit, scale=3.0, order=od, K_b=K_b, conf=True)
        want, r = want_buffers(hyps, scores, first, unit=unit, scale=3.0, order=od, K_b=K_b, conf=True)
        same_bits(got, want)
    D = r["dist"]
    assert (D == D.transpose(0, 2, 1)).all()
    real = D[:, np.arange(K), np.arange(K)] == 0
    assert real.any() and ((D >= 0) == (real[:, :, None] & real[:, None, :])).all()
    if K > 2:
        assert (D > 0).any() and (D == -1).any()


@pytest.mark.parametrize("unit", ["char", "word"])
def test_panels_and_ragged_pairs(unit):
    """257 against 257 units (past one panel of 256 columns) and 300 against 5; in word unit the rows are that many
    one-symbol words"""
    rs = np.random.RandomState(9)

    def row(n):
        syms = rs.randint(2, 6, size=n)
        if unit == "char":
            return syms.astype(np.int32)
        out = np.full(2 * n - 1, SP, dtype=np.int32)
        out[0::2] = syms
        return out
    a = row(257)
    b = a.copy()
    b[[0, 200 if unit == "char" else 400]] = 6          # a symbol that no row has: two units differ
    hyps = [[a, b], [row(300), row(5)]]
    scores = np.zeros((2, 2))
    got, first = run_mbr(hyps, scores, unit=unit, conf=True)
    want, r = want_buffers(hyps, scores, first, unit=unit, conf=True)
    same_bits(got, want)
    assert r["dist"][0, 0, 1] == 2 and r["dist"][1, 0, 1] >= 295 and r["conf_len"].tolist() == [257, 300]


def test_constructed_ties():
    chain = [[[2, 3, 4], [2, 3, 5], [2, 6, 5]], [[2], [3], [2]]]
    scores = np.zeros((2, 3))
    got, first = run_mbr(chain, scores)
    want, r = want_buffers(chain, scores, first)
    same_bits(got, want)
    assert r["order"].tolist() == [[1, 0, 2], [0, 2, 1]] and r["best"].tolist() == [1, 0]
    order = [[2, 1, 0], [1, 2, 0]]
    got, first = run_mbr(chain, scores, order=order)
    want, r = want_buffers(chain, scores, first, order=order)
    same_bits(got, want)
    assert r["order"].tolist() == [[1, 2, 0], [2, 0, 1]] and r["best"].tolist() == [1, 2]


def test_no_real_hypothesis_and_empty_batch():
    import _sctc
    hyps = [[[2, 3], [4]], [[2], [2]]]
    scores = np.array([[math.nan, -math.inf], [0.0, 0.0]])
    got, first = run_mbr(hyps, scores, K_b=[2, 0], conf=True)
    want, r = want_buffers(hyps, scores, first, K_b=[2, 0], conf=True)
    same_bits(got, want)
    assert r["best"].tolist() == [-1, -1] and (r["dist"] == -1).all()
    cfg = _sctc.MbrConfig(0, 4, 0, 0, 8, 1, 1.0, None, None, None)
    assert _sctc.lib().sctc_nbest_mbr_batch(ctypes.byref(cfg), *([None] * 11 + [0, None])) == 0


# ---- 2. general scores -------------------------------------------------------------------------------------------------

REL = 1e-12
# Seed lists chosen on the CPU (test_risk_gap_of_the_seeds_is_known_on_the_cpu_side repeats the count): at most one seed in
# ten of a list has two neighbouring model risks within 1e-9 relative in either unit.
SEEDS = {0.0: tuple(range(20)), 1.0: tuple(range(20)), 50.0: tuple(range(20))}


def general_case(seed, scale):
    """(hyps, scores, K_b) of a seed.  Scales 0 and 1: B = 3, K = 5, 17 or 40 related hypotheses.  Scale 50: one hypothesis
    takes everything and a risk is the distance to it, a small integer, so lists of 40 always hold two hypotheses as far
    from the top one; there K = 4 hypotheses that each change 0, 1, 2 or 4 words of their own in a sentence of ten, by one symbol: in both
    units the distances to the top one all differ."""
    B = 3
    if scale == 50.0:
        K = 4
        rs = np.random.RandomState(1000 + seed)
        hyps = []
        for _ in range(B):
            base = [list(rs.randint(2, 6, size=int(rs.randint(2, 4)))) for _ in range(10)]
            where, changes = list(rs.permutation(10)), rs.permutation([0, 1, 2, 4])
            row = []
            for c in changes:       # hypothesis k replaces its own c_k words of the base: D(k, j) = c_k + c_j
                words = [list(w) for w in base]
                for _ in range(int(c)):
                    w = words[where.pop()]
                    w[0] = 2 + (w[0] - 1) % 4
                row.append(np.array(sum(([SP] + w for w in words), [])[1:], dtype=np.int32))
            hyps.append(row)
    else:
        K = (5, 17, 40)[seed % 3]
        hyps, rs = random_lists(seed, B, K, 20, distinct=True)
    scores = -10.0 + 4.0 * rs.rand(B, K)
    scores[1, K // 2] = -math.inf
    return hyps, scores, [K, K, max(1, K - 3)]


def clear_risks(r, scale):
    """may `best` and `order` be compared?  At scale 0 every weight is exactly 1.0 and every sum an integer: risks tie
    exactly on both sides and the tie rule decides, so every seed is compared.  Otherwise the model's neighbouring risks
    have to be apart by more than 1e-9 relative."""
    return scale == 0.0 or M.min_risk_gap(r) > 1e-9


def rel_err(got, want):
    fin = np.isfinite(want)
    assert (got[~fin] == want[~fin]).all()
    g, w = got[fin], want[fin]
    nz = w != 0
    assert (g[~nz] == 0).all()
    return float(np.max(np.abs(g[nz] - w[nz]) / np.abs(w[nz]))) if nz.any() else 0.0


@pytest.mark.parametrize("unit", ["char", "word"])
@pytest.mark.parametrize("scale", [0.0, 1.0, 50.0])
def test_general_scores(unit, scale):
    worst, skipped, took_all = 0.0, 0, 0
    for seed in SEEDS[scale]:
        hyps, scores, K_b = general_case(seed, scale)
        B, K = len(hyps), len(hyps[0])
        got, first = run_mbr(hyps, scores, unit=unit, scale=scale, K_b=K_b, conf=True)
        want, r = want_buffers(hyps, scores, first, unit=unit, scale=scale, K_b=K_b, conf=True)
        same_bits(got, want, keys=("dist",))
        errs = [rel_err(got[k][:-TAIL], want[k][:-TAIL]) for k in ("posterior", "risk")]
        for k in ("posterior", "risk", "confidence"):
            assert (got[k][-TAIL:] == GD).all(), k
        if clear_risks(r, scale):
            # the choice, the order and so the confidences of the chosen hypothesis
            same_bits(got, want, keys=("best", "order", "conf_len"))
            errs.append(rel_err(got["confidence"][:-TAIL], want["confidence"][:-TAIL]))
        else:
            skipped += 1
        worst = max([worst] + errs)
        if scale == 0.0:        # uniform posteriors, and nothing but exact arithmetic: every buffer bit for bit
            n_real = (r["posterior"] > 0).sum(axis=1)
            for b in range(B):
                assert (r["posterior"][b][r["posterior"][b] > 0] == 1.0 / n_real[b]).all()
            same_bits(got, want)
        if scale == 50.0:
            for b in range(B):      # one hypothesis takes (almost) everything: the risk is its row of D
                top = int(np.argmax(r["posterior"][b]))
                if r["posterior"][b, top] > 1 - 1e-13:
                    took_all += 1
                    real = r["dist"][b, top] >= 0
                    np.testing.assert_allclose(got["risk"][:-TAIL].reshape(B, K)[b][real], r["dist"][b, top][real],
                                               rtol=1e-11, atol=1e-11)
    print("unit %s scale %g: worst relative error %.3g, %d of %d seeds set aside" % (unit, scale, worst, skipped,
                                                                                     len(SEEDS[scale])))
    assert worst <= REL
    assert skipped * 10 <= len(SEEDS[scale])
    assert scale != 50.0 or 2 * took_all >= 3 * len(SEEDS[scale])       # the property was looked at: half of the utterances


def test_risk_gap_of_the_seeds_is_known_on_the_cpu_side():
    """the seed lists keep within the cap at every scale and in both units (asserted again, on the device's side, in
    test_general_scores)"""
    for unit in ("char", "word"):
        for scale in (0.0, 1.0, 50.0):
            close = 0
            for seed in SEEDS[scale]:
                hyps, scores, K_b = general_case(seed, scale)
                r = M.mbr(hyps, scores, unit=unit, scale=scale, space=SP, A=8, K_b=K_b)
                close += not clear_risks(r, scale)
            assert close * 10 <= len(SEEDS[scale]), (unit, scale, close)


# ---- 3. confidences ------------------------------------------------------------------------------------------------------

def test_confidence_cases():
    w = math.exp(-1.0)
    hyps = [[[2, 3, 4], [5, 5, 5]],                 # K_b = 1: certain
            [[2, 3, 2], [2]],                       # MATCH first: the LAST x agrees, not the first
            [[2, 3], [3, 2]]]                       # a = the chosen one: x agrees (LEFT MATCH UP), not y
    scores = np.array([[0.0, 0.0], [0.0, -1.0], [0.0, 0.0]])
    got, first = run_mbr(hyps, scores, K_b=[1, 2, 2], conf=True)
    want, r = want_buffers(hyps, scores, first, K_b=[1, 2, 2], conf=True)
    same_bits(got, want, keys=("best", "order", "dist", "conf_len"))
    assert r["best"].tolist() == [0, 0, 0] and first.tolist() == [0, 3, 6, 8]
    c = got["confidence"]
    assert c[0:3].tolist() == [1.0, 1.0, 1.0]
    assert rel_err(c[3:6], np.array([1 / (1 + w), 1 / (1 + w), 1.0])) <= REL and c[5] == 1.0
    assert c[6:8].tolist() == [1.0, 0.5]
    assert (c[8:] == GD).all()
    # words: "a b" chosen, "a c", "a": the word in all three hypotheses is certain
    words = [[[2, SP, 3], [2, SP, 4], [2]]]
    got, first = run_mbr(words, np.zeros((1, 3)), unit="word", conf=True)
    want, r = want_buffers(words, np.zeros((1, 3)), first, unit="word", conf=True)
    same_bits(got, want)
    assert got["confidence"][:2].tolist() == [1.0, 1 / 3] and got["conf_len"][0] == 2


def test_operation_table_in_the_workspace():
    """256 against 256 units: 64 x 64 words of operations and the counts do not fit the 16 KB slot; the neighbour
    utterance's table (40 x 40 units) stays on chip"""
    rs = np.random.RandomState(21)
    a = rs.randint(2, 5, size=256).astype(np.int32)
    b = a.copy()
    b[rs.permutation(256)[:40]] = 5
    b = np.delete(b, [3, 77])
    b = np.concatenate([b, [2, 2]]).astype(np.int32)
    c = rs.randint(2, 5, size=40).astype(np.int32)
    hyps = [[a, b, a[:200]], [c, c[::-1].copy(), c[:7]]]
    scores = np.zeros((2, 3))
    got, first = run_mbr(hyps, scores, conf=True)
    want, r = want_buffers(hyps, scores, first, conf=True)
    same_bits(got, want)
    assert r["conf_len"][0] in (256, 200) and 0 < got["confidence"][:first[1]].min() < 1


# ---- 4. composition ----------------------------------------------------------------------------------------------------

def test_search_second_pass_and_mbr_in_place():
    """decode_beam_batch(device=True) -> rescore_nbest(device=True) -> mbr_nbest(device=True) on the search's tensors
    equals the route through host lists bit for bit, and a second call gives the same bits"""
    import ctc_fast
    rs = np.random.RandomState(17)
    T_b, K, A = [40, 26, 33], 6, 35
    lps = [bt.peaked(rs, A, T) for T in T_b]
    import torch
    dev = torch.from_numpy(np.concatenate([lp.T for lp in lps], axis=0)).cuda()
    trip = ctc_fast.decode_beam_batch(dev, lengths=T_b, beam=10, nbest=K, device=True)
    order_d, resc_d = ctc_fast.rescore_nbest(dev, trip, lengths=T_b, beta=0.3, device=True)
    hyps, first_scores = ctc_fast.decode_beam_batch(lps, beam=10, nbest=K)
    order_h, resc_h = ctc_fast.rescore_nbest(lps, hyps, beta=0.3, scores=first_scores)
    assert resc_d.cpu().numpy().tobytes() == resc_h.tobytes()
    flat = np.concatenate([h for row in hyps for h in row])
    space = int(np.bincount(flat, minlength=A)[1:].argmax()) + 1
    for unit in ("char", "word"):
        kw = dict(unit=unit, scale=0.7, space=space, A=A, confidences=True, distances=True)
        d1 = ctc_fast.mbr_nbest(trip, resc_d, order=order_d, device=True, lengths=T_b, **kw)
        d2 = ctc_fast.mbr_nbest(trip, resc_d, order=order_d, device=True, lengths=T_b, **kw)
        h = ctc_fast.mbr_nbest(hyps, resc_h, order=order_h, **kw)
        m = M.mbr(hyps, resc_h, order=order_h, unit=unit, scale=0.7, space=space, A=A, confidences=True)
        assert (m["dist"] == h["dist"]).all()
        for k in ("best", "posterior", "risk", "order", "dist"):
            a, b = d1[k].cpu().numpy(), d2[k].cpu().numpy()
            assert a.tobytes() == b.tobytes() == h[k].tobytes(), (unit, k)
        (c1, n1), (c2, n2) = d1["confidence"], d2["confidence"]
        assert c1.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes() and (n1 == n2).all()
        starts = np.concatenate([[0], np.cumsum([max(((len(x) + 1) // 2 if unit == "word" else len(x)) for x in row)
                                                 for row in hyps])])
        c1, n1 = c1.cpu().numpy(), n1.cpu().numpy()
        for b in range(len(hyps)):
            assert c1[starts[b]:starts[b] + n1[b]].tobytes() == h["confidence"][b].tobytes()
            assert len(h["confidence"][b]) == len(m["confidence"][b])
        assert (h["best"] >= 0).all()
