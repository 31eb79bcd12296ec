"""tests/rescore_model.py checked on the CPU against cases worked out by hand, and mutation-checked: a model with the
tie rule swapped, or with the sum reassociated, must be told apart from the model by these same cases."""
import numpy as np

from tests import rescore_model as M

NEG = M.NEG


def case():
    """B = 4, K = 5: ties, -inf totals, a status != 0, K_b < K, K_b = 0"""
    total = np.array([[-10.0, -9.0, -9.0, -12.0, -9.0],          # 1, 2 and 4 tie: order 1, 2, 4
                      [-5.0, NEG, -4.0, -4.5, -3.0],             # rank 1 cannot be aligned (status 1): last of the real
                      [-7.0, -6.0, -1.0, -1.0, -1.0],            # K_b = 2: ranks 2.. are no hypotheses however good
                      [-1.0, -2.0, -3.0, -4.0, -5.0]])           # K_b = 0
    status = np.array([[0, 0, 0, 0, 0], [0, 1, 0, 2, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    K_b = [5, 5, 2, 0]
    return total, status, K_b


def test_ties_neg_inf_status_and_k_b():
    total, status, K_b = case()
    U = np.zeros((4, 5), dtype=np.int32)
    order, res = M.rank(total, status, None, U, K_b, 1.0, 0.0)
    assert order.tolist() == [[1, 2, 4, 0, 3],
                              [4, 2, 0, 1, 3],       # 1 (status 1) and 3 (status 2) at -inf: tie, lower rank first
                              [1, 0, 2, 3, 4],
                              [0, 1, 2, 3, 4]]
    assert res[1].tolist() == [-5.0, NEG, -4.0, NEG, -3.0]
    assert res[2].tolist() == [-7.0, -6.0, NEG, NEG, NEG]
    assert (res[3] == NEG).all()


def test_first_pass_scores_mark_the_ranks_beyond_the_beam():
    total, status, _ = case()
    U = np.zeros((4, 5), dtype=np.int32)
    first = np.array([[0.0, -1.0, -2.0, NEG, NEG], [0.0, -1.0, -2.0, -3.0, -4.0], [NEG] * 5, [0.0, NEG, -1.0, -2.0, -3.0]])
    order, res = M.rank(total, status, None, U, [5, 5, 5, 5], 1.0, 0.0, first=first)
    assert order[0].tolist() == [1, 2, 0, 3, 4] and res[0, 3] == NEG and res[0, 4] == NEG
    assert order[2].tolist() == [0, 1, 2, 3, 4] and (res[2] == NEG).all()
    assert order[3].tolist() == [0, 1, 2, 3, 4] and res[3].tolist() == [-1.0, NEG, NEG, NEG, NEG]
    # K_b and the scores together: the smaller count holds
    order, res = M.rank(total, status, None, U, [2, 5, 5, 5], 1.0, 0.0, first=first)
    assert order[0].tolist() == [1, 0, 2, 3, 4]


def test_lm_and_length_terms():
    total = np.array([[-10.0, -11.0, -12.0]])
    lm = np.array([[-8.0, -4.0, -1.0]])
    U = np.array([[3, 4, 2]])
    order, res = M.rank(total, np.zeros((1, 3), int), lm, U, [3], 0.5, 1.5)
    assert res[0].tolist() == [-10.0 - 4.0 + 4.5, -11.0 - 2.0 + 6.0, -12.0 - 0.5 + 3.0]
    assert order[0].tolist() == [1, 0, 2]                        # -9.5, -7.0, -9.5: 0 and 2 tie


def inexact_case():
    """values at which (t + a * l) + b * U and t + (a * l + b * U) round differently"""
    rs = np.random.RandomState(7)
    total = -rs.rand(3, 6) * 300
    lm = -rs.rand(3, 6) * 80
    U = rs.randint(1, 60, size=(3, 6))
    return total, lm, U


def test_mutations_are_detected():
    total, status, K_b = case()
    U = np.zeros((4, 5), dtype=np.int32)
    good = M.rank(total, status, None, U, K_b, 1.0, 0.0)
    swapped = M.rank(total, status, None, U, K_b, 1.0, 0.0, tie="high")
    assert not np.array_equal(good[0], swapped[0])               # the tie rule shows in the order
    assert swapped[0][0].tolist() == [4, 2, 1, 0, 3]
    np.testing.assert_array_equal(good[1], swapped[1])
    t, lm, Ux = inexact_case()
    a = M.rank(t, np.zeros((3, 6), int), lm, Ux, [6, 6, 6], 0.7, 0.3)
    b = M.rank(t, np.zeros((3, 6), int), lm, Ux, [6, 6, 6], 0.7, 0.3, assoc="right")
    assert not np.array_equal(a[1], b[1])                        # the association shows in the bits
    assert np.abs(a[1] - b[1]).max() < 1e-12
    # and the model is the operation order of score_sentences: total + alpha * lmv + beta * len
    want = np.array([[t[i, k] + 0.7 * lm[i, k] + 0.3 * int(Ux[i, k]) for k in range(6)] for i in range(3)])
    np.testing.assert_array_equal(a[1], want)
