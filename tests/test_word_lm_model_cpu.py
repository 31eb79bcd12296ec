"""The word-LM second pass on the CPU: tests/word_lm_model.py against the LM classes' own sentence
scores, ctc_fast.word_lm_sentence_scores against the model, and the mutation checks of the edge rows."""
import os
import types

import numpy as np
import pytest

from tests import word_lm_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
A = 35
_CACHE = {}


def setup(kind):
    """(chars, words, tree, lm) of "bg" (decoder.lm.LM) or an n-gram order 2..4; the lexicon of the GPU tests"""
    import _sctc  # noqa: F401  (puts the package on the path)
    from decoder import decoder_utils, lm as lm_mod, ngram_lm, prefixTree
    if kind not in _CACHE:
        chars = decoder_utils.load_chars(os.path.join(GOLDEN, "chars.txt"))
        words = decoder_utils.load_words(os.path.join(GOLDEN, "words_bg.txt")) + [wm.LONG_WORD]
        lm = lm_mod.LM(os.path.join(GOLDEN, "lm_word_2g.arpa")) if kind == "bg" else \
            ngram_lm.NgramLM(os.path.join(GOLDEN, "lm_word_4g.arpa"), kind)
        tree = prefixTree.PrefixTree(chars, words, lm, specials=["[laughter]", "[noise]"])
        _CACHE[kind] = (chars, words, tree, lm)
    return _CACHE[kind]


def sentences(words, seed, n=20):
    rs = np.random.RandomState(seed)
    short = [w for w in words if len(w) < 10]
    return [" ".join(short[rs.randint(len(short))] for _ in range(rs.randint(1, 9))) for _ in range(n)]


def running32(terms):
    s = np.float32(0.0)
    for t in terms:
        s = np.float32(s + t)
    return s


def test_bigram_model_with_eos_is_score_bg():
    chars, words, tree, lm = setup("bg")
    for text in sentences(words, 1):
        got = wm.score_row(wm.spell(chars, text), tree, lm, A, eos=True)
        assert got["status"] == 0 and got["words"] == len(text.split()) and got["oov"] == 0
        want = lm.score_bg(text)
        assert running32(got["terms"]).tobytes() == np.float32(want).tobytes(), text


@pytest.mark.parametrize("order", [2, 3, 4])
def test_ngram_model_without_eos_is_score(order):
    chars, words, tree, lm = setup(order)
    for text in sentences(words, order):
        got = wm.score_row(wm.spell(chars, text), tree, lm, A)
        assert got["status"] == 0 and got["oov"] == 0
        assert running32(got["terms"]).tobytes() == np.float32(lm.score(text)).tobytes(), text


def all_rows(chars, words):
    return [r for _, r in wm.edge_rows(chars)] + wm.random_rows(chars, words[:120], 5)


@pytest.mark.parametrize("kind", ["bg", 2, 3, 4])
@pytest.mark.parametrize("eos", [False, True])
@pytest.mark.parametrize("final_word", [False, True])
def test_host_route_equals_the_model(kind, eos, final_word):
    import ctc_fast
    chars, words, tree, lm = setup(kind)
    rows = all_rows(chars, words) + [[2, 0, 3], [2, A, 3]]
    lex = types.SimpleNamespace(tree=tree, lm=lm, A=A)
    sums, counts, status = ctc_fast.word_lm_sentence_scores(rows, lex, eos=eos, final_word=final_word)
    w_sums, w_counts, w_status, _, _ = wm.score_rows(rows, tree, lm, A, eos=eos, final_word=final_word)
    assert sums.dtype == np.float64 and counts.dtype == np.int32 and status.dtype == np.int32
    assert sums.tobytes() == w_sums.tobytes()
    np.testing.assert_array_equal(counts, w_counts)
    np.testing.assert_array_equal(status, w_status)
    assert status[-2:].tolist() == [2, 2] and (status[:-2] == 0).all() and np.isfinite(sums[:-2]).all()


def test_generator_rows_hold_enough_of_both_kinds():
    chars, words, tree, lm = setup("bg")
    rows = wm.random_rows(chars, words[:120], 5)
    toks = [t for r in rows for t, _ in wm.tokens_of(r, tree.space)]
    known = sum(1 for t in toks if (lambda n: n is not None and n.isWord)(wm.walk(tree, t)[0]))
    assert len(toks) >= 60
    assert known >= 0.5 * len(toks) and len(toks) - known >= 0.2 * len(toks), (known, len(toks))


def test_edge_rows_are_what_their_names_say():
    chars, words, tree, lm = setup("bg")
    rows = dict(wm.edge_rows(chars))
    sp = tree.space
    assert len(rows["8191 symbols"]) == 8191
    cross = wm.tokens_of(rows["a token across symbols 63 / 64"], sp)
    start = 2 * 31
    assert rows["a token across symbols 63 / 64"][start - 1] == sp and len(cross[31][0]) == 5       # symbols 62..66
    third = [t for t, _ in wm.tokens_of(rows["200 symbols, off the tree at the third"], sp) if len(t) == 200]
    last = [t for t, _ in wm.tokens_of(rows["200 symbols, off the tree at the last"], sp) if len(t) == 200]
    assert wm.walk(tree, third[0]) == (None, 2) and wm.walk(tree, last[0]) == (None, 199)
    seventy = wm.score_row(rows["70 one-letter words"], tree, lm, A)
    assert seventy["words"] == 70 and seventy["oov"] == 0
    aoe, unk = lm.word_to_int["aoe"], lm.unk
    assert lm.bg[(aoe, unk)] == 0.0 and aoe in wm.score_row(rows["aoe, then an OOV"], tree, lm, A)["ids"]
    ng = setup(4)[3]
    assert ng.ngrams[(ng.unk, ng.word_to_int["oot"])][0] == 0.0


@pytest.mark.parametrize("mutation", wm.MUTATIONS)
def test_every_mutation_fails_an_edge_row(mutation):
    """a model that drops the final word, omits <s>, skips an OOV, takes the bigram's listed 0.0 for a value or counts
    </s> as a word differs from the model on at least one edge row"""
    chars, words, tree, lm = setup("bg")
    differs = 0
    for _, row in wm.edge_rows(chars)[:10]:
        for eos in (False, True):
            good = wm.score_row(row, tree, lm, A, eos=eos)
            bad = wm.score_row(row, tree, lm, A, eos=eos, mutate=mutation)
            differs += (good["sum"], good["words"], good["oov"]) != (bad["sum"], bad["words"], bad["oov"])
    assert differs >= 1


def test_no_unk_gives_status_3(tmp_path):
    from decoder import lm as lm_mod, prefixTree
    chars, words, _, _ = setup("bg")
    path = tmp_path / "no_unk.arpa"
    path.write_text("\\data\\\nngram 1=4\nngram 2=1\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-0.7\ta\t-0.3\n"
                    "-0.9\teat\t-0.2\n\n\\2-grams:\n-0.4\ta eat\n\n\\end\\\n")
    lm = lm_mod.LM(str(path))
    tree = prefixTree.PrefixTree(chars, ["a", "eat"], lm)
    ok = wm.score_row(wm.spell(chars, "a eat"), tree, lm, A)
    bad = wm.score_row(wm.spell(chars, "a to eat"), tree, lm, A)
    assert ok["status"] == 0 and np.isfinite(ok["sum"])
    assert bad["status"] == 3 and bad["sum"] == wm.NEG and (bad["words"], bad["oov"]) == (3, 1)
    # the OOV token is the unfinished last one: no word, no status 3
    assert wm.score_row(wm.spell(chars, "a to"), tree, lm, A, final_word=False)["status"] == 0
