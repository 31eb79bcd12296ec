"""The rank rule of n-best rescoring with the word-LM term (tests/word_lm_model.rank) in NumPy
float64: the operation order, ties, K_b, -inf, and that without the word term it is tests/rescore_model.rank."""
import numpy as np

from tests import rescore_model
from tests import word_lm_model as wm

NEG = float("-inf")


def case(seed=4, B=5, K=6):
    rs = np.random.RandomState(seed)
    total = -rs.rand(B, K) * 30
    lm = -rs.rand(B, K) * 12
    U = rs.randint(0, 20, size=(B, K))
    status = (rs.rand(B, K) < 0.15).astype(np.int32)
    wsum = -rs.rand(B, K) * 25
    wcount = np.stack([rs.randint(0, 8, size=(B, K)), rs.randint(0, 3, size=(B, K))], axis=-1).astype(np.int32)
    wstatus = np.where(rs.rand(B, K) < 0.15, 3, 0).astype(np.int32)
    wsum[wstatus != 0] = NEG
    return total, status, lm, U, wsum, wcount, wstatus


def test_operation_order_is_left_to_right():
    got = wm.combine(0.1, 0.2, 3, 0.3, 0.7, -1.1, 4, 0, 1.3, 0.9)
    want = np.float64(np.float64(np.float64(0.1) + np.float64(0.3) * np.float64(0.2)) + np.float64(0.7) * np.float64(3.0)) \
        + np.float64(np.float64(1.3) * np.float64(-1.1) + np.float64(0.9) * np.float64(4.0))
    assert got == float(want)
    # a reassociation is visible on such numbers: the rule is not "any order"
    rs = np.random.RandomState(0)
    seen = 0
    for _ in range(200):
        t, l, ws = -rs.rand(3) * 40
        left = wm.combine(t, l, 7, 0.7, 0.4, ws, 3, 0, 1.3, 0.9)
        flat = (((t + 0.7 * l) + 0.4 * 7.0) + 1.3 * ws) + 0.9 * 3.0
        seen += left != flat
    assert seen > 0


def test_word_status_is_minus_infinity_without_a_product():
    with np.errstate(all="raise"):
        assert wm.combine(-3.0, -1.0, 2, 1.0, 0.0, NEG, 2, 3, 0.0, 0.0) == NEG      # word_alpha 0: no 0 * -inf = nan
    assert wm.combine(-3.0, -1.0, 2, 1.0, 0.0, -2.0, 2, 0, 0.0, 0.0) == (-3.0 + -1.0) + 0.0


def test_rank_with_zero_word_weights_is_the_rule_without_words():
    total, status, lm, U, wsum, wcount, _ = case()
    K_b = [6, 4, 0, 6, 1]
    clean = np.zeros_like(status)
    wsum = np.where(np.isfinite(wsum), wsum, -1.0)
    for lmv in (lm, None):
        want = rescore_model.rank(total, status, lmv, U, K_b, 0.7, 0.4)
        got = wm.rank(total, status, lmv, U, K_b, 0.7, 0.4, wsum, wcount, clean, 0.0, 0.0)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_rank_ties_K_b_first_and_minus_infinity():
    total, status, lm, U, wsum, wcount, wstatus = case()
    total[0, :] = -5.0
    lm[0, :] = -1.0
    U[0, :] = 3
    status[0, :] = 0
    wsum[0, :] = -2.0
    wcount[0, :, 0] = 2
    wstatus[0, :] = 0
    wstatus[0, 2] = 3                                   # one of the tied hypotheses cannot be scored
    K_b = [6, 4, 0, 6, 1]
    first = np.zeros_like(total)
    first[3, 2:] = NEG                                  # the first pass filled ranks 2.. of utterance 3
    order, res = wm.rank(total, status, lm, U, K_b, 0.7, 0.4, wsum, wcount, wstatus, 1.3, 0.9, first=first)
    assert order[0].tolist() == [0, 1, 3, 4, 5, 2] and res[0, 2] == NEG and len(set(res[0, [0, 1, 3, 4, 5]])) == 1
    assert order[2].tolist() == list(range(6)) and (res[2] == NEG).all()            # K_b = 0
    assert sorted(order[1][:4].tolist()) == [0, 1, 2, 3] and order[1][4:].tolist() == [4, 5] and (res[1, 4:] == NEG).all()
    assert sorted(order[3][:2].tolist()) == [0, 1] and order[3][2:].tolist() == [2, 3, 4, 5] and (res[3, 2:] == NEG).all()
    for b in range(5):
        kb = rescore_model.real_count(K_b[b], first[b])
        vals = res[b][order[b][:kb]]
        assert (vals[:-1] >= vals[1:]).all()
        for k in range(kb):
            ok = status[b, k] == 0 and wstatus[b, k] == 0
            assert np.isfinite(res[b, k]) == ok
    # the word term moves the order: with it off, some utterance ranks differently
    plain = rescore_model.rank(total, status, lm, U, K_b, 0.7, 0.4, first=first)[0]
    assert (plain != order).any()
