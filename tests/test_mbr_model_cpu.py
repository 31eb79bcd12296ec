"""tests/mbr_model.py against hand-worked cases, and every mutation switch of the model against at
least one of them: a rule that the model had wrong, or that a mutation did not touch, would show here and not on the
GPU, where the device is compared with the model."""
import math

import numpy as np
import pytest

from tests import mbr_model as M

SP = 1      # the space symbol of the cases


def ids_of(rows, groups, **kw):
    ids, counts, status = M.intern(rows, groups, SP, 8, **kw)
    return [v.tolist() for v in ids], counts.tolist(), status.tolist()


def test_tokens_are_maximal_runs():
    assert M.tokens([], SP) == []
    assert M.tokens([SP, SP], SP) == []
    assert M.tokens([SP, 2, SP, SP, 3, 4, SP], SP) == [(2,), (3, 4)]
    assert M.tokens([2, 3], SP) == [(2, 3)]


def test_intern_hand_cases():
    # one row: "ab abc ab" -> the third word is the first again
    assert ids_of([[2, 3, SP, 2, 3, 4, SP, 2, 3]], [0, 1]) == ([[0, 1, 0]], [3], [0])
    # the same word in another row of the group keeps the first row's number; numbering runs on through the group
    assert ids_of([[2, 3], [4, SP, 2, 3], [4]], [0, 3]) == ([[0], [1, 0], [1]], [1, 2, 1], [0, 0, 0])
    # groups are worlds of their own
    assert ids_of([[2, 3], [4, SP, 2, 3]], [0, 1, 2]) == ([[0], [0, 1]], [1, 2], [0, 0])
    # words that differ in the last symbol only
    assert ids_of([[2, 3, 4, SP, 2, 3, 5]], [0, 1]) == ([[0, 1]], [2], [0])
    # a label outside [1, A): status 2, no words, and the numbering of the group goes on without the row
    assert ids_of([[2], [2, 9], [3, SP, 2]], [0, 3]) == ([[0], [], [1, 0]], [1, 0, 2], [0, 2, 0])
    assert ids_of([[0, 2]], [0, 1])[2] == [2]
    # an empty group and an empty row
    assert ids_of([[]], [0, 0, 1]) == ([[]], [0], [0])


def test_intern_mutations_change_a_case():
    prefix = [[2, 3, SP, 2, 3, 4]]
    assert ids_of(prefix, [0, 1])[0] == [[0, 1]]
    assert ids_of(prefix, [0, 1], mut_prefix=True)[0] == [[0, 0]]
    spaces = [[SP, 2, SP, SP, 3, SP]]
    assert ids_of(spaces, [0, 1])[:2] == ([[0, 1]], [2])
    assert ids_of(spaces, [0, 1], mut_empty_words=True)[1] == [5]


def test_intern_buffers_layout():
    flat, counts, status, first = M.intern_buffers([[2, SP, 3], [], [2, 2, 2], [3]], [0, 4], SP, 8, fill=-5)
    assert first.tolist() == [0, 2, 2, 4, 5]
    # (2,2,2) is a new word, the group's token number 2; the second slot of its row is not written; (3) is token 1
    assert flat.tolist() == [0, 1, 2, -5, 1] and counts.tolist() == [2, 0, 1, 1]


# three hypotheses in symbols: d01 = 1, d02 = 2, d12 = 1
CHAIN = [[[2, 3, 4], [2, 3, 5], [2, 6, 5]]]


def test_equal_scores_are_exact():
    r = M.mbr(CHAIN, [[-3.0, -3.0, -3.0]], unit="char", scale=7.0)
    assert r["dist"][0].tolist() == [[0, 1, 2], [1, 0, 1], [2, 1, 0]]
    assert r["posterior"][0].tolist() == [1 / 3, 1 / 3, 1 / 3]
    assert r["risk"][0].tolist() == [3 / 3, 2 / 3, 3 / 3]
    assert r["best"].tolist() == [1] and r["order"][0].tolist() == [1, 0, 2]


def test_tie_rule_and_its_mutation():
    order = [[2, 1, 0]]     # the ranking of the second pass puts hypothesis 2 first
    r = M.mbr(CHAIN, [[-3.0, -3.0, -3.0]], unit="char", order=order)
    assert r["order"][0].tolist() == [1, 2, 0]
    assert M.mbr(CHAIN, [[-3.0, -3.0, -3.0]], unit="char", order=order, mut_tie=True)["order"][0].tolist() == [1, 0, 2]
    # a tie for the first place
    two = [[[2], [3]]]
    assert M.mbr(two, [[0.0, 0.0]], unit="char")["best"].tolist() == [0]
    assert M.mbr(two, [[0.0, 0.0]], unit="char", order=[[1, 0]])["best"].tolist() == [1]
    assert M.mbr(two, [[0.0, 0.0]], unit="char", order=[[1, 0]], mut_tie=True)["best"].tolist() == [0]


def test_ranks_that_are_not_real():
    hyps = [[[2, 3], [2], [2, 3, 4], [5]]]
    r = M.mbr(hyps, [[0.0, -math.inf, 0.0, 0.0]], unit="char", K_b=[3])
    assert r["dist"][0].tolist() == [[0, -1, 1, -1], [-1, -1, -1, -1], [1, -1, 0, -1], [-1, -1, -1, -1]]
    assert r["posterior"][0].tolist() == [0.5, 0.0, 0.5, 0.0]
    assert r["risk"][0].tolist() == [0.5, math.inf, 0.5, math.inf]
    assert r["best"].tolist() == [0] and r["order"][0].tolist() == [0, 2, 1, 3]
    nan = M.mbr(hyps, [[math.nan, 0.0, math.nan, 0.0]], unit="char", K_b=[3])
    assert nan["best"].tolist() == [1] and nan["order"][0].tolist() == [1, 0, 2, 3]
    assert nan["risk"][0].tolist() == [math.inf, 0.0, math.inf, math.inf]
    none = M.mbr(hyps, [[0.0] * 4], unit="char", K_b=[0], confidences=True)
    assert none["best"].tolist() == [-1] and none["order"][0].tolist() == [0, 1, 2, 3]
    assert (none["dist"] == -1).all() and none["conf_len"].tolist() == [0]


def test_weights_scale_and_the_order_of_the_sums():
    hyps = [[[2], [3], [4], [5]]]       # every distance is 1
    sc = [[0.0, -36.5, -36.6, -50.0]]
    w1, w2, w3 = math.exp(-36.5), math.exp(-36.6), math.exp(-50.0)
    Z = ((1.0 + w1) + w2) + w3
    r = M.mbr(hyps, sc, unit="char")
    assert r["posterior"][0].tolist() == [1.0 / Z, w1 / Z, w2 / Z, w3 / Z]
    # hypothesis 3: 1 * 1 + w1 * 1 + w2 * 1 in ascending j, then the division
    assert r["risk"][0, 3] == ((1.0 + w1) + w2) / Z
    assert r["best"].tolist() == [0]
    assert M.mbr(hyps, sc, unit="char", mut_descending=True)["risk"][0, 3] == ((w2 + w1) + 1.0) / Z != r["risk"][0, 3]
    nf = M.mbr(hyps, sc, unit="char", mut_normalise_first=True)["risk"][0, 3]
    assert nf == (1.0 / Z + w1 / Z) + w2 / Z != r["risk"][0, 3]
    # scale 0: uniform posteriors; a large scale: the top hypothesis takes everything and the risk is its row of D
    assert M.mbr(hyps, sc, unit="char", scale=0.0)["posterior"][0].tolist() == [0.25] * 4
    big = M.mbr(CHAIN, [[-1.0, 0.0, -2.0]], unit="char", scale=1000.0)
    assert big["posterior"][0].tolist() == [0.0, 1.0, 0.0] and big["risk"][0].tolist() == [1.0, 0.0, 1.0]


def test_word_unit_interns_per_utterance():
    # "ab cd" / "ab ce" / "ab": in words d01 = 1, d02 = 1, d12 = 1; in symbols 1, 3, 3
    hyps = [[[2, 3, SP, 4, 5], [2, 3, SP, 4, 6], [2, 3]]]
    r = M.mbr(hyps, [[0.0] * 3], unit="word", space=SP, A=8)
    assert r["dist"][0].tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert M.mbr(hyps, [[0.0] * 3], unit="char")["dist"][0].tolist() == [[0, 1, 3], [1, 0, 3], [3, 3, 0]]
    # the prefix mutation merges "ab" and "abc"
    pre = [[[2, 3], [2, 3, 4]]]
    assert M.mbr(pre, [[0.0, 0.0]], unit="word", space=SP, A=8)["dist"][0, 0, 1] == 1
    assert M.mbr(pre, [[0.0, 0.0]], unit="word", space=SP, A=8, mut_prefix=True)["dist"][0, 0, 1] == 0
    dbl = [[[2, SP, SP, 3], [2, SP, 3]]]
    assert M.mbr(dbl, [[0.0, 0.0]], unit="word", space=SP, A=8)["dist"][0, 0, 1] == 0
    assert M.mbr(dbl, [[0.0, 0.0]], unit="word", space=SP, A=8, mut_empty_words=True)["dist"][0, 0, 1] == 1


def test_confidences():
    # one real hypothesis: every unit is certain
    one = M.mbr([[[2, 3, 4], [5]]], [[0.0, 0.0]], unit="char", K_b=[1], confidences=True)
    assert one["confidence"][0].tolist() == [1.0, 1.0, 1.0] and one["conf_len"].tolist() == [3]
    # equal scores, words: "a b" chosen (rank tie), "a c", "a": the first word is in all three, the second in one
    hyps = [[[2, SP, 3], [2, SP, 4], [2]]]
    r = M.mbr(hyps, [[0.0] * 3], unit="word", space=SP, A=8, confidences=True)
    assert r["best"].tolist() == [0]
    assert r["confidence"][0].tolist() == [3 / 3, 1 / 3]
    # the path's tie order: x y x against x matches the LAST x (MATCH is tried first at the end of both)
    tie = M.mbr([[[2, 3, 2], [2]]], [[0.0, -1.0]], unit="char", confidences=True)
    w = math.exp(-1.0)
    assert tie["best"].tolist() == [0]
    assert tie["confidence"][0].tolist() == [1.0 / (1.0 + w), 1.0 / (1.0 + w), (1.0 + w) / (1.0 + w)]
    # a = chosen: "xy" against "yx" matches x (LEFT, MATCH, UP); with a = other the match lands on y
    swap = [[[2, 3], [3, 2]]]
    r = M.mbr(swap, [[0.0, 0.0]], unit="char", confidences=True)
    assert r["best"].tolist() == [0] and r["confidence"][0].tolist() == [1.0, 0.5]
    assert M.mbr(swap, [[0.0, 0.0]], unit="char", confidences=True, mut_conf_other=True)["confidence"][0].tolist() == [0.5, 1.0]


SWAP = [[[2, 3], [3, 2]]]
# switch -> (arguments of M.mbr for a listed case, the output that the switch has to change)
MUTATION_CASES = {
    "mut_tie": (dict(hyps=CHAIN, scores=[[-3.0] * 3], unit="char", order=[[2, 1, 0]]), "order"),
    "mut_descending": (dict(hyps=[[[2], [3], [4], [5]]], scores=[[0.0, -36.5, -36.6, -50.0]], unit="char"), "risk"),
    "mut_normalise_first": (dict(hyps=[[[2], [3], [4], [5]]], scores=[[0.0, -36.5, -36.6, -50.0]], unit="char"), "risk"),
    "mut_conf_other": (dict(hyps=SWAP, scores=[[0.0, 0.0]], unit="char", confidences=True), "confidence"),
    "mut_prefix": (dict(hyps=[[[2, 3], [2, 3, 4]]], scores=[[0.0, 0.0]], unit="word", space=SP, A=8), "dist"),
    "mut_empty_words": (dict(hyps=[[[2, SP, SP, 3], [2, SP, 3]]], scores=[[0.0, 0.0]], unit="word", space=SP, A=8), "dist"),
}


@pytest.mark.parametrize("mut", sorted(MUTATION_CASES))
def test_every_mutation_changes_a_listed_case(mut):
    import inspect
    assert sorted(MUTATION_CASES) == sorted(p for p in inspect.signature(M.mbr).parameters if p.startswith("mut_"))
    kw, key = MUTATION_CASES[mut]
    plain, mutated = M.mbr(**kw)[key], M.mbr(**dict(kw, **{mut: True}))[key]
    assert np.asarray(plain).tobytes() != np.asarray(mutated).tobytes()


def test_min_risk_gap():
    r = M.mbr(CHAIN, [[-3.0, -3.0, -3.0]], unit="char")
    assert M.min_risk_gap(r) == 0.0
    assert np.isinf(M.min_risk_gap(M.mbr([[[2]]], [[0.0]], unit="char")))
