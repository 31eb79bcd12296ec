"""GPU checks of sctc_word_lm_score_batch (csrc/word_lm_score.hip) through ctc_fast.word_lm_score_batch:
sums, counts, status, terms and word ids equal tests/word_lm_model.py bit for bit, for the bigram handle and the n-gram
handles of order 2, 3 and 4."""
import numpy as np
import pytest

from tests import word_lm_model as wm
from tests.test_word_lm_model_cpu import A, setup

pytestmark = pytest.mark.gpu

KINDS = ["bg", 2, 3, 4]
_DEV = {}


def lexicon(kind):
    import ctc_fast
    if kind not in _DEV:
        _, _, tree, lm = setup(kind)
        _DEV[kind] = ctc_fast.DecodeLexicon.from_tree(tree, lm, A)
    return _DEV[kind]


def check(got, rows, kind, eos=False, final_word=True):
    """(sums, counts, status, terms, words) of the list route against the model, equal bits"""
    _, _, tree, lm = setup(kind)
    sums, counts, status, terms, ids = got
    w_sums, w_counts, w_status, w_terms, w_ids = wm.score_rows(rows, tree, lm, A, eos=eos, final_word=final_word)
    np.testing.assert_array_equal(status, w_status)
    np.testing.assert_array_equal(counts, w_counts)
    assert sums.dtype == np.float64 and sums.tobytes() == w_sums.tobytes()
    for n in range(len(rows)):
        assert terms[n].dtype == np.float32 and ids[n].dtype == np.int32
        assert terms[n].tobytes() == np.asarray(w_terms[n], dtype=np.float32).tobytes(), n
        assert ids[n].tolist() == w_ids[n], n
    return w_sums, w_counts, w_status


@pytest.mark.parametrize("kind", KINDS)
def test_edge_rows_in_one_batch(kind):
    import torch
    import ctc_fast
    chars, words, tree, lm = setup(kind)
    names, rows = zip(*wm.edge_rows(chars))
    got = ctc_fast.word_lm_score_batch(list(rows), lexicon(kind), terms=True, words=True)
    sums, counts, status = check(got, rows, kind)
    assert (status == 0).all() and sums[0] == 0.0 and sums[1] == 0.0 and counts[:2].tolist() == [[0, 0], [0, 0]]
    assert counts[names.index("leading, trailing and double spaces")].tolist() == [3, 0]
    assert counts[names.index("a single special")].tolist() == [1, 0]
    assert counts[names.index("70 one-letter words")].tolist() == [70, 0]
    assert counts[names.index("200 symbols, off the tree at the third")].tolist() == [3, 1]
    assert counts[names.index("200 symbols, off the tree at the last")].tolist() == [3, 1]
    assert counts[names.index("8191 symbols"), 0] > 1500 and counts[names.index("8191 symbols"), 1] > 300
    # two sequences sharing one ids range, a third inside it, read in place
    row = rows[names.index("a token across symbols 63 / 64")]
    ids = torch.tensor([1] * 5 + list(row), dtype=torch.int32).cuda()
    shared = [row, row, row[2:40]]
    triple = (ids, [len(r) for r in shared], [5, 5, 7])
    d = ctc_fast.word_lm_score_batch(triple, lexicon(kind), terms=True, words=True)
    check(d, shared, kind)
    assert d[0][0] == d[0][1] == sums[names.index("a token across symbols 63 / 64")]


@pytest.mark.parametrize("kind", KINDS)
def test_random_rows_flags_and_a_bad_row_between_good_ones(kind):
    import ctc_fast
    chars, words, tree, lm = setup(kind)
    rows = wm.random_rows(chars, words[:120], 5)
    rows[7] = rows[6][:3] + [A] + rows[6][3:]           # outside the alphabet
    rows[11] = [2, 0, 3]                                # the blank
    rows[12] = [2, 3, -4]
    for eos in (False, True):
        for final_word in (False, True):
            got = ctc_fast.word_lm_score_batch(rows, lexicon(kind), terms=True, words=True, eos=eos, final_word=final_word)
            sums, counts, status = check(got, rows, kind, eos=eos, final_word=final_word)
            assert status[[7, 11, 12]].tolist() == [2, 2, 2] and (sums[[7, 11, 12]] == wm.NEG).all()
            assert (np.delete(status, [7, 11, 12]) == 0).all() and counts[[7, 11, 12]].sum() == 0
    # the good rows are what they are without the bad ones next to them
    good = [r for i, r in enumerate(rows) if i not in (7, 11, 12)]
    alone = ctc_fast.word_lm_score_batch(good, lexicon(kind), eos=True)
    assert alone[0].tobytes() == np.delete(sums, [7, 11, 12]).tobytes()


def test_lm_without_unk_gives_status_3(tmp_path):
    import ctc_fast
    from decoder import lm as lm_mod, prefixTree
    chars = setup("bg")[0]
    path = tmp_path / "no_unk.arpa"
    path.write_text("\\data\\\nngram 1=4\nngram 2=1\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-0.7\ta\t-0.3\n"
                    "-0.9\teat\t-0.2\n\n\\2-grams:\n-0.4\ta eat\n\n\\end\\\n")
    lm = lm_mod.LM(str(path))
    tree = prefixTree.PrefixTree(chars, ["a", "eat"], lm)
    lex = ctc_fast.DecodeLexicon.from_tree(tree, lm, A)
    rows = [wm.spell(chars, t) for t in ("a eat", "a to eat", "eat a", "a to")]
    for final_word, want in ((True, [0, 3, 0, 3]), (False, [0, 3, 0, 0])):
        sums, counts, status, terms, ids = ctc_fast.word_lm_score_batch(rows, lex, terms=True, words=True, eos=True,
                                                                        final_word=final_word)
        w = wm.score_rows(rows, tree, lm, A, eos=True, final_word=final_word)
        assert status.tolist() == want and status.tolist() == w[2].tolist()
        assert sums.tobytes() == w[0].tobytes() and counts.tolist() == w[1].tolist()
        assert sums[1] == wm.NEG and counts[1].tolist() == [3 if final_word else 2, 1] and len(terms[1]) == 0 and len(ids[1]) == 0
        assert [t.tolist() for t in terms] == [[float(x) for x in r] for r in w[3]]
    lex.close()


def test_device_route_on_the_ids_of_a_search_and_two_equal_runs():
    import torch
    import ctc_fast
    from tests import beam_trace as bt
    kind = 3
    rs = np.random.RandomState(12)
    T_b = [40, 25, 33]
    K = 4
    lps = [bt.peaked(rs, A, T) for T in T_b]
    ids, lens, scores = ctc_fast.decode_beam_batch(lps, beam=8, nbest=K, device=True)
    before = ids.clone()
    U = lens.cpu().numpy()
    base = np.concatenate([[0], np.cumsum(T_b)])
    offs = np.asarray([K * base[b] + n * T_b[b] for b in range(3) for n in range(K)], dtype=np.int64)
    out = ctc_fast.word_lm_score_batch((ids, U, offs), lexicon(kind), terms=True, words=True, device=True)
    assert all(t.is_cuda for t in out) and torch.equal(ids, before)
    host_ids = ids.cpu().numpy()
    rows = [host_ids[o:o + u].tolist() for o, u in zip(offs, U)]
    _, _, tree, lm = setup(kind)
    w_sums, w_counts, w_status, w_terms, w_ids = wm.score_rows(rows, tree, lm, A)
    assert out[0].cpu().numpy().tobytes() == w_sums.tobytes() and w_counts[:, 0].sum() > 0
    np.testing.assert_array_equal(out[1].cpu().numpy(), w_counts)
    np.testing.assert_array_equal(out[2].cpu().numpy(), w_status)
    first = np.concatenate([[0], np.cumsum((U + 1) // 2 + 1)])
    terms, wids = out[3].cpu().numpy(), out[4].cpu().numpy()
    assert terms.shape[0] == first[-1] == wids.shape[0]
    for n in range(len(rows)):
        assert terms[first[n]:first[n] + len(w_terms[n])].tobytes() == np.asarray(w_terms[n], np.float32).tobytes()
        assert wids[first[n]:first[n] + len(w_ids[n])].tolist() == w_ids[n]
    again = ctc_fast.word_lm_score_batch((ids, U, offs), lexicon(kind), terms=True, words=True, device=True)
    for a, b in zip(out, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["bg", 4])
def test_word_lm_perplexity_against_the_model(kind):
    import ctc_fast
    chars, words, tree, lm = setup(kind)
    rows = [r for r in wm.random_rows(chars, words[:120], 9) if r]
    for eos in (True, False):
        ppl, n, n_oov = ctc_fast.word_lm_perplexity(rows, lexicon(kind), eos=eos)
        w_sums, w_counts, w_status, _, _ = wm.score_rows(rows, tree, lm, A, eos=eos)
        want_n = int(w_counts[:, 0].sum()) + (len(rows) if eos else 0)
        assert (n, n_oov) == (want_n, int(w_counts[:, 1].sum())) and n_oov > 0
        assert ppl == float(np.exp(-float(w_sums.sum()) / want_n))
    with pytest.raises(ValueError):
        ctc_fast.word_lm_perplexity(rows + [[2, 0]], lexicon(kind))
    with pytest.raises(ValueError):
        ctc_fast.word_lm_perplexity([[]], lexicon(kind), eos=False)


def test_lm_perplexity_tool_with_a_word_lm(tmp_path, capsys):
    import os
    from tests.test_word_lm_model_cpu import GOLDEN
    from tools import lm_perplexity
    chars, words, _, _ = setup("bg")
    names = {v: k for k, v in chars.items()}
    rows = [wm.spell(chars, t) for t in ("eat a ntttn", "to zzq oot", "[laughter] an")]
    text = tmp_path / "text.txt"
    text.write_text("".join(" ".join(names[c] for c in r) + "\n" for r in rows))
    pp = lm_perplexity.main(["--text", str(text), "--chars", os.path.join(GOLDEN, "chars.txt"), "--word-lm",
                             os.path.join(GOLDEN, "lm_word_4g.arpa"), "--words", os.path.join(GOLDEN, "words_bg.txt"),
                             "--word-lm-order", "3", "--specials", "[laughter]", "[noise]"])
    _, _, tree, lm = setup(3)
    sums, counts, _, _, _ = wm.score_rows(rows, tree, lm, A, eos=True)
    assert pp == float(np.exp(-float(sums.sum()) / (int(counts[:, 0].sum()) + 3)))
    assert "word perplexity" in capsys.readouterr().out and int(counts[:, 1].sum()) == 1
    with pytest.raises(SystemExit):
        lm_perplexity.main(["--text", str(text), "--chars", os.path.join(GOLDEN, "chars.txt"), "--word-lm", "x.arpa"])


def test_empty_batch_and_workspace_check():
    import ctypes
    import torch
    import _sctc
    import ctc_fast
    lex = lexicon("bg")
    sums, counts, status = ctc_fast.word_lm_score_batch([], lex)
    assert sums.shape == (0,) and counts.shape == (0, 2) and status.shape == (0,)
    U = np.asarray([4, 0], dtype=np.int32)
    off = np.zeros(2, dtype=np.int64)
    cfg = _sctc.WordLmScoreConfig(2, A, lex.handle, int(lex.lm.unk), int(lex.lm.end), 0, 0, _sctc.i32(U), _sctc.i64(off))
    need = ctypes.c_size_t(0)
    L = _sctc.lib()
    _sctc.check(L.sctc_word_lm_score_workspace_bytes(ctypes.byref(cfg), ctypes.byref(need)), "word_lm_score")
    assert need.value == 256 + 256
    buf = torch.zeros(64, dtype=torch.int32).cuda()
    p = buf.data_ptr()
    ws = torch.empty(need.value, dtype=torch.uint8).cuda()
    rc = L.sctc_word_lm_score_batch(ctypes.byref(cfg), p, None, None, p, p, p, ws.data_ptr(), need.value - 1,
                                    _sctc.current_stream_ptr())
    assert rc == -3                                     # SCTC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert not buf.any()
