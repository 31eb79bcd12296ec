"""CPU-side checks of the lexicon-constrained word-bigram decoder: the Python
restatement (tests/lex_beam_model.py) against the reference's own results
(tests/golden/decode_bg_ref.npz), the LM of decoder/lm.py against values worked out from the ARPA
text by lm.cpp's formula, the prefix tree and its flattening, and the argument errors of the new C
entry points (none of which needs a GPU)."""
import ctypes
import os

import numpy as np
import pytest

from tests import lex_beam_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHARS = os.path.join(GOLDEN, "chars.txt")
WORDS = os.path.join(GOLDEN, "words_bg.txt")
ARPA = os.path.join(GOLDEN, "lm_word_2g.arpa")

N_SMALL_ALPHA, N_SMALL = 120, 40       # tests/golden/make_golden_decode_bg.py
SCALE = float(np.float32(np.log(10.0)))


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    ge._paths()
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


def fixture_lexicon(words, A, size):
    """(words, specials) of a fixture case, as the generator's lexicon_of"""
    if A == 8:
        return words[:N_SMALL if size == "small" else N_SMALL_ALPHA], ["[laughter]"]
    sp = ["[laughter]", "[noise]"] + (["[vocalized-noise]"] if A >= 34 else [])
    return words[:N_SMALL if size == "small" else len(words)], sp


def load_objects(sctc):
    from decoder import decoder_utils, lm as lm_mod
    return decoder_utils.load_chars(CHARS), decoder_utils.load_words(WORDS), lm_mod.LM(ARPA)


def arpa_text():
    """(unigram rows {word: (text prob, text back-off or None)}, bigram rows {(w1, w2): text})"""
    uni, bi, sec = {}, {}, 0
    order = []
    for line in open(ARPA):
        s = line.split()
        if not s:
            continue
        if s[0].startswith("\\"):
            sec = {"\\1-grams:": 1, "\\2-grams:": 2}.get(s[0], 0)
        elif sec == 1:
            uni[s[1]] = (s[0], s[2] if len(s) > 2 else None)
            order.append(s[1])
        elif sec == 2:
            bi[(s[1], s[2])] = s[0]
    return uni, bi, order


def val(text):
    return np.float32(SCALE * float(text))


def test_restatement_reproduces_the_reference(sctc):
    from decoder import prefixTree
    chars, words, lm = load_objects(sctc)
    z = np.load(os.path.join(GOLDEN, "decode_bg_ref.npz"))
    n = int(z["n"])
    assert n >= 40
    trees, skipped = {}, 0
    for i in range(n):
        A, T, beam, alpha, beta = z["cfg%d" % i]
        A, T, beam = int(A), int(T), int(beam)
        size = str(z["lex%d" % i])
        if (A, size) not in trees:
            lex, sp = fixture_lexicon(words, A, size)
            trees[(A, size)] = lex_beam_model.from_objects(prefixTree.PrefixTree(chars, lex, lm, specials=sp), lm, A)
        child, word, bg, start, space = trees[(A, size)]
        top = lex_beam_model.decode(z["lp%d" % i], child, word, bg, start, space, beam, alpha, beta, nbest=2)
        ref = float(z["score%d" % i])
        assert abs(top[0][1] - ref) <= 1e-9 * abs(ref), (i, top[0][1], ref)
        margin = top[0][1] - top[1][1] if len(top) > 1 else np.inf
        m_ref = float(z["margin%d" % i])
        assert margin == m_ref or abs(margin - m_ref) <= 1e-9, (i, margin, m_ref)
        if margin >= 1e-6:
            assert list(top[0][0]) == list(z["hyp%d" % i]), i
        else:
            skipped += 1
    assert skipped <= 0.05 * n        # the cap of DESIGN.md §4.6


def test_lm_follows_lm_cpp(sctc):
    _, _, lm = load_objects(sctc)
    uni, bi, order = arpa_text()
    assert [lm.word_to_int[w] for w in order] == list(range(len(order)))       # ids: 1-gram order
    assert lm.start == lm.word_to_int["<s>"] and lm.end == lm.word_to_int["</s>"]
    assert lm.unk == lm.word_to_int["<UNK>"]
    for w in order[:50]:
        assert lm.ug_prob(lm.word_to_int[w]) == val(uni[w][0])
    # a listed bigram
    (w1, w2), text = next((k, t) for k, t in bi.items() if float(t) != 0.0)
    got = lm.bg_prob(lm.word_to_int[w1], lm.word_to_int[w2])
    assert got == val(text) and got.dtype == np.float32
    # a pair that is not listed: float32 sum of back-off and unigram
    w1 = next(w for w in order[5:] if uni[w][1] is not None)
    w2 = next(w for w in order[5:] if (w1, w) not in bi)
    want = np.float32(val(uni[w1][1]) + val(uni[w2][0]))
    assert lm.bg_prob(lm.word_to_int[w1], lm.word_to_int[w2]) == want
    # a unigram without a back-off column: back-off 0
    w1 = next(w for w in order[5:] if uni[w][1] is None)
    w2 = next(w for w in order[5:] if (w1, w) not in bi)
    assert lm.bg_prob(lm.word_to_int[w1], lm.word_to_int[w2]) == val(uni[w2][0])
    # the quirk: a listed bigram of exactly 0.0 counts as missing (lm.cpp:121-125)
    zeros = [k for k, t in bi.items() if float(t) == 0.0]
    assert zeros
    for w1, w2 in zeros[:10]:
        want = np.float32(val(uni[w1][1] or "0") + val(uni[w2][0]))
        assert want != 0.0 and lm.bg_prob(lm.word_to_int[w1], lm.word_to_int[w2]) == want
    # an unknown word is <UNK>
    assert lm.get_word_id("no-such-word") == lm.unk
    # a sentence score: the running float32 sum over <s> .. </s>
    a, b = order[5], order[6]
    s = np.float32(0.0)
    for x, y in ((lm.start, lm.word_to_int[a]), (lm.word_to_int[a], lm.word_to_int[b]), (lm.word_to_int[b], lm.end)):
        s = np.float32(s + lm.bg_prob(x, y))
    assert lm.score_bg("%s %s" % (a, b)) == s


def test_lm_without_unk_rejects_unknown_words(sctc, tmp_path):
    from decoder import lm as lm_mod
    p = tmp_path / "tiny.arpa"
    p.write_text("\\data\\\nngram 1=3\nngram 2=1\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-0.3\ta\t-0.2\n\n"
                 "\\2-grams:\n-0.1\t<s> a\n\n\\3-grams:\n-0.7\t<s> a a\n\n\\end\\\n")
    lm = lm_mod.LM(str(p))
    assert lm.unk is None and lm.num_words == 3 and len(lm.bg) == 1      # the 3-gram section is ignored
    with pytest.raises(ValueError):
        lm.get_word_id("b")
    p2 = tmp_path / "lower.arpa"
    p2.write_text(p.read_text().replace("ngram 1=3", "ngram 1=4").replace("-0.3\ta\t-0.2", "-0.3\ta\t-0.2\n-2.0\t<unk>"))
    assert lm_mod.LM(str(p2)).get_word_id("b") == 3


def test_bigram_table_packing(sctc):
    import arpa_lm
    _, _, lm = load_objects(sctc)
    keys, vals = lm.pack_bigrams()
    cap = keys.shape[0]
    assert cap & (cap - 1) == 0 and (keys != np.uint64(0xFFFFFFFFFFFFFFFF)).sum() == len(lm.bg) <= cap // 2
    for (w1, w2), v in list(lm.bg.items())[::37]:
        key = np.uint64((w1 << 32) | w2)
        s = int(arpa_lm.mix64(np.array([key], dtype=np.uint64))[0]) & (cap - 1)
        while keys[s] != key:
            assert keys[s] != np.uint64(0xFFFFFFFFFFFFFFFF)
            s = (s + 1) & (cap - 1)
        assert vals[s] == v


def test_prefix_tree_flattening_round_trips(sctc):
    from decoder import prefixTree
    chars, words, lm = load_objects(sctc)
    A = 35
    specials = ["[laughter]", "[noise]", "[vocalized-noise]"]
    tree = prefixTree.PrefixTree(chars, words, lm, specials=specials)
    assert tree.space == chars["[space]"] == 1
    assert tree.root.isPrefix and not tree.root.isWord
    child, word = tree.flatten(A)
    assert child.dtype == np.int32 and word.dtype == np.int32 and child.shape == (word.shape[0], A)
    ends = {}
    for w in words:                                   # every word spells a path to a node with its id
        n = 0
        for ch in w:
            n = child[n, chars[ch]]
            assert n > 0
        assert word[n] == lm.get_word_id(w)
        ends[int(n)] = w
    for tok in specials:                              # specials hang off the root
        n = child[0, chars[tok]]
        assert n > 0 and word[n] == lm.get_word_id(tok) and (child[n] < 0).all()
        ends[int(n)] = tok
    assert sorted(np.nonzero(word >= 0)[0]) == sorted(ends)           # no other node is a word
    assert word[0] == -1 and (child[:, 0] < 0).all() and (child[:, tree.space] < 0).all()
    # every node but the root has exactly one parent, and every node is reachable
    kids = child[child >= 0]
    assert sorted(kids) == list(range(1, child.shape[0]))
    # a word that is also a prefix of a longer word is both isWord and isPrefix
    both = [w for w in words if any(v != w and v.startswith(w) for v in words)]
    assert both
    node = tree.root
    for ch in both[0]:
        node = node.children[chars[ch]]
    assert node.isWord and node.isPrefix
    # a missing child answers like the reference's defaultdict, and is not kept
    assert not tree.root.children[chars["&"]].isPrefix and chars["&"] not in tree.root.children
    with pytest.raises(ValueError):
        prefixTree.PrefixTree({"a": 2, "[space]": 1, "b": 1}, ["ab"], lm)     # a word through the space symbol
    with pytest.raises(ValueError):
        tree.flatten(8)                               # symbols beyond the alphabet


def test_decoder_utils(sctc, tmp_path):
    from decoder import decoder_utils as du
    chars = du.load_chars(CHARS)
    assert chars["[space]"] == 1 and chars["a"] == 2
    assert du.load_words(WORDS)[0] and len(du.load_words(WORDS)) == 360
    toks = du.int_to_char([2, 5, 1, 32, 1, 6, 7], chars)
    assert toks == ["a", "t", "[space]", "[noise]", "[space]", "o", "n"]
    assert du.collapse_seq(toks) == "at [noise] on"


def test_bg_decoder_argument_checks(sctc):
    from decoder import bg_decoder
    good = np.asfortranarray(np.zeros((8, 4)))
    with pytest.raises(TypeError):
        bg_decoder.decode_bg_lm(None, None, None)
    with pytest.raises(ValueError):
        bg_decoder.decode_bg_lm(good.astype(np.float32), None, None)
    with pytest.raises(ValueError):
        bg_decoder.decode_bg_lm(np.ascontiguousarray(good), None, None)
    with pytest.raises(ValueError):
        bg_decoder.decode_bg_lm(np.zeros(4), None, None)
    with pytest.raises(OverflowError):
        bg_decoder.decode_bg_lm(good, None, None, beam=-1)


def test_argument_errors_need_no_gpu(sctc):
    """everything that can be rejected is rejected before a device is touched"""
    L = sctc.lib()
    A, nodes = 4, 3
    child = np.full((nodes, A), -1, dtype=np.int32)
    child[0, 2], child[1, 3] = 1, 2
    word = np.array([-1, -1, 1], dtype=np.int32)
    ug = np.zeros(3, dtype=np.float32)
    keys = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    vals = np.zeros(4, dtype=np.float32)
    h = ctypes.c_void_p()

    def create(child=child, word=word, nodes=nodes, A=A, space=1, n_words=3, keys=keys, cap=4, start=0):
        return L.sctc_lexicon_create(child.ctypes.data, word.ctypes.data, nodes, A, space, ug.ctypes.data,
                                     ug.ctypes.data, n_words, keys.ctypes.data, vals.ctypes.data, cap, start,
                                     ctypes.byref(h))
    assert L.sctc_lexicon_create(None, word.ctypes.data, nodes, A, 1, ug.ctypes.data, ug.ctypes.data, 3,
                                 keys.ctypes.data, vals.ctypes.data, 4, 0, ctypes.byref(h)) == -1
    assert create(A=1) == -1 and create(A=257) == -1
    assert create(space=0) == -1 and create(space=A) == -1
    assert create(nodes=0) == -1
    assert create(start=3) == -1 and create(start=-1) == -1
    assert create(cap=3) == -1 and b"power of two" in L.sctc_last_error()
    bad = child.copy()
    bad[1, 3] = 3                                   # a child outside the tree
    assert create(child=bad) == -1
    bad = child.copy()
    bad[1, 1] = 2                                   # a child for the space
    assert create(child=bad) == -1
    bad = child.copy()
    bad[1, 3] = 0                                   # an edge back to the root
    assert create(child=bad) == -1
    assert create(word=np.array([-1, -1, 3], dtype=np.int32)) == -1          # a word id outside the vocabulary
    assert create(word=np.array([0, -1, 1], dtype=np.int32)) == -1 and b"root" in L.sctc_last_error()
    full = np.array([1, 2, (1 << 32) | 1, 5], dtype=np.uint64)
    assert create(keys=full) == -1                  # no empty slot
    assert create(keys=np.array([7 << 32, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF],
                                dtype=np.uint64)) == -1                      # a bigram of an unknown word
    assert h.value is None
    assert L.sctc_lexicon_destroy(None) == 0 and L.sctc_lexicon_bytes(None) == 0
    # the decode entry points: a config without a lexicon, then nothing else is looked at
    T = np.array([5], dtype=np.int32)
    off = np.zeros(1, dtype=np.int64)
    cfg = sctc.LexBeamConfig(1, A, sctc.F32, 8, 1, 1, A, sctc.i32(T), sctc.i64(off), 1.0, 0.0, None)
    assert L.sctc_ctc_lexbeam_workspace_bytes(ctypes.byref(cfg)) == 0
    assert b"lexicon" in L.sctc_last_error()
    assert L.sctc_ctc_lexbeam_workspace_bytes(None) == 0
    assert L.sctc_ctc_lexbeam_decode_batch(ctypes.byref(cfg), None, None, None, None, None, 0, None) == -1
    with pytest.raises(ValueError):
        sctc.check(-1, "x")


def test_struct_mirror_matches_the_header(sctc, tmp_path):
    import subprocess
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(sctc_lexbeam_config),'
                    ' offsetof(sctc_lexbeam_config, space), offsetof(sctc_lexbeam_config, alpha),'
                    ' offsetof(sctc_lexbeam_config, lexicon)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    C = sctc.LexBeamConfig
    assert got == [ctypes.sizeof(C), C.space.offset, C.alpha.offset, C.lexicon.offset]


def test_python_surface_rejects_before_the_device(sctc):
    import ctc_fast
    lp = np.zeros((8, 3))
    with pytest.raises(ValueError):
        ctc_fast.decode_lexicon_beam_batch([lp], lexicon=None)
    with pytest.raises(ValueError):
        ctc_fast.decode_lexicon_beam_batch([lp], lexicon="words.txt")
