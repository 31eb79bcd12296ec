"""CPU-side checks of the lexicon decoder's word n-gram LM: decoder/ngram_lm.py
against a brute-force back-off rule on tuples of strings (tests/lex_ngram_beam_model.py), its packed
table walked the way the device walks it, order 2 against decoder/lm.py, the restatement at order 2
against tests/lex_beam_model.py on the reference's 42 inputs, the mistakes the cases would notice,
and the argument errors of sctc_lexicon_create_ngram (none of which needs a GPU)."""
import ctypes
import os

import numpy as np
import pytest

from tests import lex_beam_model
from tests import lex_ngram_beam_model as ngm
from tests.test_decode_bg_cpu import ARPA, CHARS, GOLDEN, WORDS, fixture_lexicon

ARPA4 = os.path.join(GOLDEN, "lm_word_4g.arpa")
EMPTY = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    ge._paths()
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


def filtered_bigram_file(directory):
    """a copy of lm_word_2g.arpa without its listed bigrams of exactly 0.000000, the count fixed: on it
    decoder.lm.LM's 0.0 quirk never applies, so it and an order-2 NgramLM define the same function"""
    path = os.path.join(str(directory), "lm_word_2g_nozero.arpa")
    if os.path.exists(path):
        return path
    out, sec, kept = [], 0, 0
    for line in open(ARPA).read().split("\n"):
        s = line.split()
        if s and s[0].startswith("\\"):
            sec = 2 if s[0] == "\\2-grams:" else 0
        elif s and sec == 2:
            if float(s[0]) == 0.0:
                continue
            kept += 1
        out.append(line)
    text = "\n".join(out)
    old = next(l for l in out if l.startswith("ngram 2="))
    assert int(old.split("=")[1]) == kept + 60
    with open(path, "w") as f:
        f.write(text.replace(old, "ngram 2=%d" % kept))
    return path


def pairs_for(brute, order, seed, count=2000):
    """(history words, word): every listed n-gram of length 2..order as (context, last word) -- the
    suffix-incomplete ones among them -- each of those again behind one more history word, and
    ``count`` seeded random pairs, half of them within the words the n-grams favour"""
    rs = np.random.RandomState(seed)
    words = brute.words
    out = [(g[:-1], g[-1]) for g in brute.grams if len(g) >= 2]
    out += [((words[rs.randint(len(words))],) + g[:-1], g[-1]) for g in brute.grams if len(g) >= 2]
    for _ in range(count):
        hi = 62 if rs.rand() < 0.5 else len(words)
        h = tuple(words[i] for i in rs.randint(0, hi, size=rs.randint(1, 5)))
        out.append((h, words[rs.randint(1, hi)]))
    return out


def suffix_incomplete(brute):
    return [g for g in brute.grams if len(g) >= 3 and g[1:] not in brute.grams]


# ---- the fixture ---------------------------------------------------------------------------------

def test_fixture_is_what_the_generator_promises():
    assert os.path.getsize(ARPA4) <= 150 * 1024
    b = ngm.BruteLM(ARPA4, 4)
    by_len = {n: [g for g in b.grams if len(g) == n] for n in (1, 2, 3, 4)}
    assert all(by_len[n] for n in by_len)
    for w in ("<s>", "</s>", "<UNK>", "[noise]", "[laughter]"):
        assert (w,) in b.grams
    lexicon = [l.strip() for l in open(WORDS) if l.strip()]
    assert 10 <= sum((w,) not in b.grams for w in lexicon) <= 14
    rows, sec = {1: [], 2: [], 3: [], 4: []}, 0
    for line in open(ARPA4):
        f = line.split()
        if f and f[0].startswith("\\"):
            sec = int(f[0][1]) if f[0].endswith("-grams:") else 0
        elif f and sec:
            rows[sec].append(f)
    for n in (1, 2, 3):                                   # with and without the back-off column
        assert any(len(r) == n + 1 for r in rows[n]) and any(len(r) == n + 2 for r in rows[n])
    assert all(len(r) == 5 for r in rows[4])
    for n in (2, 3, 4):
        assert sum(b.grams[g][0] == 0.0 for g in by_len[n]) >= 20          # listed, exactly 0.000000
        assert all(g[:-1] in b.grams for g in by_len[n])                   # prefix closure
    inc = suffix_incomplete(b)
    assert sum(len(g) == 3 for g in inc) >= 30 and sum(len(g) == 4 for g in inc) >= 30


# ---- the host LM ---------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [2, 3, 4])
def test_prob_equals_the_brute_force_bit_for_bit(sctc, order):
    from decoder import ngram_lm
    lm = ngram_lm.NgramLM(ARPA4, order)
    brute = ngm.BruteLM(ARPA4, order)
    assert lm.order == order and lm.num_words == len(brute.words)
    assert [lm.word_to_int[w] for w in brute.words] == list(range(len(brute.words)))      # ids: 1-gram order
    assert (lm.start, lm.end, lm.unk) == (brute.ids["<s>"], brute.ids["</s>"], brute.ids["<UNK>"])
    assert len(lm.ngrams) == sum(len(g) >= 2 for g in brute.grams)                        # higher sections ignored
    table = lm.pack()
    pairs = pairs_for(brute, order, seed=order)
    assert len(pairs) >= 2000 + 2 * len(lm.ngrams)
    if order >= 3:
        assert len(suffix_incomplete(brute)) >= 30
    backed_off = stopped = 0
    for i, (h, w) in enumerate(pairs):
        want = brute.prob(h, w)
        hid = [brute.ids[x] for x in h]
        got = lm.prob(hid, brute.ids[w])
        assert got.dtype == np.float32 and got == want, (h, w, got, want)
        # the packed table, walked as the device walks it: every pair
        assert ngram_lm.walk_packed(table, lm.ug, lm.bo, hid, brute.ids[w], order) == want, (h, w)
        ht = h[-(order - 1):]
        backed_off += ht + (w,) not in brute.grams
        # the back-off sum stops early: a context of the history is missing below its full length
        stopped += any(ht[k:] not in brute.grams for k in range(1, len(ht) - 1)) if len(ht) > 2 else 0
    assert backed_off > 500 and (order < 4 or stopped > 100)
    for g in suffix_incomplete(brute):                    # every one of them, through the table as well
        hid, w = [brute.ids[x] for x in g[:-1]], brute.ids[g[-1]]
        assert ngram_lm.walk_packed(table, lm.ug, lm.bo, hid, w, order) == brute.prob(g[:-1], g[-1]) == lm.prob(hid, w)


def test_packed_table_layout(sctc):
    from decoder import ngram_lm
    import arpa_lm
    lm = ngram_lm.NgramLM(ARPA4, 4)
    keys, vals, bos, ids, contexts = lm.pack()
    cap = keys.shape[0]
    assert cap & (cap - 1) == 0 and (keys != np.uint64(EMPTY)).sum() == len(lm.ngrams) <= cap // 2
    assert contexts == sum(len(g) < 4 for g in lm.ngrams)
    used = ids[keys != np.uint64(EMPTY)]
    assert sorted(used[used >= 0]) == list(range(lm.num_words, lm.num_words + contexts))
    assert (used < 0).sum() == sum(len(g) == 4 for g in lm.ngrams)
    for g in lm.ngrams:                                    # chain to the n-gram's slot from its oldest word
        cid = g[0]
        for w in g[1:]:
            s = ngram_lm.find_packed((keys, vals, bos, ids, contexts), cid, w)
            assert s >= 0
            cid = int(ids[s])
        assert (vals[s], bos[s]) == lm.ngrams[g] and (cid == -1) == (len(g) == 4)
        key = np.array([keys[s]], dtype=np.uint64)
        home = int(arpa_lm.mix64(key)[0]) & (cap - 1)
        assert all(keys[(home + d) & (cap - 1)] != np.uint64(EMPTY) for d in range((s - home) & (cap - 1)))


def test_order_2_is_the_bigram_lm_without_its_quirk(sctc, tmp_path):
    from decoder import lm as lm_mod, ngram_lm
    path = filtered_bigram_file(tmp_path)
    old, new = lm_mod.LM(path), ngram_lm.NgramLM(path, 2)
    assert ngram_lm.NgramLM(path).order == 2
    assert len(old.bg) == len(new.ngrams) == 2540 and not any(v == 0.0 for v in old.bg.values())
    rs = np.random.RandomState(60)
    ws = [old.start] + [int(w) for w in rs.choice(np.arange(1, old.num_words), size=59, replace=False)]
    listed = 0
    for w1 in ws:
        for w2 in ws:
            a, b = new.prob((w1,), w2), old.bg_prob(w1, w2)
            assert a == b and a.dtype == b.dtype == np.float32, (w1, w2)
            listed += (w1, w2) in old.bg
    assert listed > 5
    for (w1, w2) in list(old.bg)[::7]:
        assert new.prob((5, w1), w2) == old.bg_prob(w1, w2)          # older history is dropped at order 2
    # the quirk itself stays where it was: on the unfiltered file the two differ exactly on the zeros
    old_q, new_q = lm_mod.LM(ARPA), ngram_lm.NgramLM(ARPA, 2)
    zeros = [k for k, v in old_q.bg.items() if v == 0.0]
    assert len(zeros) == 60
    for w1, w2 in zeros:
        assert new_q.prob((w1,), w2) == 0.0 != old_q.bg_prob(w1, w2)


def test_score_word_ids_and_the_tree(sctc, tmp_path):
    from decoder import decoder_utils, ngram_lm, prefixTree
    lm = ngram_lm.NgramLM(ARPA4, 4)
    brute = ngm.BruteLM(ARPA4, 4)
    g = next(g for g in brute.grams if len(g) == 4 and g[0] != "<s>" and "</s>" not in g)
    sent = list(g) + ["no-such-word", g[1]]
    total, hist = np.float32(0.0), ["<s>"]
    for w in sent:
        w = w if w in brute.ids else "<UNK>"
        total = np.float32(total + brute.prob(hist, w))
        hist.append(w)
    assert lm.score(" ".join(sent)) == total and lm.score("").dtype == np.float32
    assert lm.get_word_id("no-such-word") == lm.unk
    chars, words = decoder_utils.load_chars(CHARS), decoder_utils.load_words(WORDS)
    tree = prefixTree.PrefixTree(chars, words, lm, specials=["[laughter]", "[noise]"])
    child, word = tree.flatten(35)
    assert (word >= 0).sum() == len(words) + 2 and (word[word >= 0] == lm.unk).sum() == 12
    tiny = tmp_path / "tiny.arpa"
    tiny.write_text("\\data\\\nngram 1=3\nngram 2=1\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-0.3\ta\t-0.2\n\n"
                    "\\2-grams:\n-0.1\t<s> a\n\n\\end\\\n")
    with pytest.raises(ValueError):
        ngram_lm.NgramLM(str(tiny)).get_word_id("b")                  # neither <UNK> nor <unk>


def test_loader_rejects_what_it_cannot_represent(sctc, tmp_path):
    from decoder import ngram_lm
    head = ("\\data\\\nngram 1=5\nngram 2=2\nngram 3=1\n\n\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-0.3\ta\t-0.2\n"
            "-0.4\tb\t-0.1\n-2\t<unk>\n\n\\2-grams:\n-0.1\t<s> a\t-0.3\n-0.2\tb a\n\n\\3-grams:\n")
    good = tmp_path / "good.arpa"
    good.write_text(head + "-0.7\t<s> a b\n\n\\end\\\n")              # suffix 'a b' is not listed: accepted
    lm = ngram_lm.NgramLM(str(good))
    # 'a b' misses first, so the listed '<s> a b' is never reached: b's unigram, then the back-offs of 'a', '<s> a'
    assert lm.order == 3 and lm.prob((0, 2), 3) == np.float32(np.float32(ngm.val("-0.4") + ngm.val("-0.2")) + ngm.val("-0.3"))
    assert lm.prob((3, 2), 3) == np.float32(np.float32(ngm.val("-0.4") + ngm.val("-0.2")))   # 'b a' has no back-off
    bad = tmp_path / "bad.arpa"
    bad.write_text(head + "-0.7\ta b a\n\n\\end\\\n")                 # prefix 'a b' is not listed
    with pytest.raises(ValueError, match="a b a"):
        ngram_lm.NgramLM(str(bad))
    assert ngram_lm.NgramLM(str(bad), 2).order == 2                   # the section above the order is not read
    unknown = tmp_path / "unknown.arpa"
    unknown.write_text(head + "-0.7\t<s> a c\n\n\\end\\\n")
    with pytest.raises(ValueError, match="<s> a c"):
        ngram_lm.NgramLM(str(unknown))
    with pytest.raises(ValueError):
        ngram_lm.NgramLM(ARPA4, order=5)                              # above the file's highest section
    for order in (1, 6):
        with pytest.raises(ValueError):
            ngram_lm.NgramLM(ARPA4, order=order)


# ---- the restatement -----------------------------------------------------------------------------

def test_restatement_at_order_2_is_the_bigram_restatement(sctc, tmp_path):
    from decoder import decoder_utils, lm as lm_mod, ngram_lm, prefixTree
    path = filtered_bigram_file(tmp_path)
    old, new = lm_mod.LM(path), ngram_lm.NgramLM(path, 2)
    chars, words = decoder_utils.load_chars(CHARS), decoder_utils.load_words(WORDS)
    z = np.load(os.path.join(GOLDEN, "decode_bg_ref.npz"))
    n = int(z["n"])
    assert n == 42
    trees = {}
    for i in range(n):
        A, T, beam, alpha, beta = z["cfg%d" % i]
        A, T, beam = int(A), int(T), int(beam)
        size = str(z["lex%d" % i])
        if (A, size) not in trees:
            lex, sp = fixture_lexicon(words, A, size)
            trees[(A, size)] = prefixTree.PrefixTree(chars, lex, new, specials=sp).flatten(A)
        child, word = trees[(A, size)]
        nb = min(beam, 8)
        a = lex_beam_model.decode(z["lp%d" % i], child, word, old.bg_prob, old.start, 1, beam, alpha, beta, nbest=nb)
        b = ngm.decode(z["lp%d" % i], child, word, new.prob, new.start, 1, 2, beam, alpha, beta, nbest=nb)
        assert a == b, i


def forced(chars, sentence, tail=(), seed=0):
    """one finite symbol per frame along the sentence's spelling, then the frames of ``tail``"""
    rs = np.random.RandomState(seed)
    syms = []
    for k, w in enumerate(sentence):
        syms += ([1] if k else []) + ([chars[w]] if w.startswith("[") else [chars[ch] for ch in w])
    frames = []
    for s in syms:
        if frames and frames[-1] == s:
            frames.append(0)
        frames.append(s)
    lp = np.full((35, len(frames) + len(tail)), -np.inf)
    lp[frames, np.arange(len(frames))] = -(0.05 + 2.0 * rs.rand(len(frames)))
    for k, col in enumerate(tail):
        for s, v in col.items():
            lp[s, len(frames) + k] = v
    return lp, syms


def mutation_cases(brute):
    """{mutation: (sentence, order)} chosen from the listed n-grams so that the mistake changes the last
    word's LM value"""
    lexicon = set(l.strip() for l in open(WORDS) if l.strip()) | {"[noise]", "[laughter]"}
    ok = lambda g: all(w in lexicon for w in g)
    tri = [g for g in brute.grams if len(g) == 3 and ok(g)]
    out = {}
    # a b c listed, b c not: stopping at the first miss gives the unigram and back-offs, going on the trigram
    out["no_stop_at_first_miss"] = (next(g for g in tri if g[1:] not in brute.grams), 3)
    # two non-zero back-offs whose float32 sum depends on the order
    for g in (g for g in brute.grams if len(g) == 3 and ok(g)):
        for w in sorted(lexicon & set(brute.ids)):
            if (g[-1], w) in brute.grams or g + (w,) in brute.grams or g[1:] not in brute.grams:
                continue
            p = brute.grams[(w,)][0]
            t = [brute.grams[g[2:]][1], brute.grams[g[1:]][1], brute.grams[g][1]]
            fwd = np.float32(np.float32(np.float32(p + t[0]) + t[1]) + t[2])
            rev = np.float32(np.float32(np.float32(p + t[2]) + t[1]) + t[0])
            if fwd != rev:
                out["backoffs_longest_first"] = (g + (w,), 4)
                break
        if "backoffs_longest_first" in out:
            break
    # at order 3 a history of three words: untruncated, the listed trigram context adds its back-off
    out["history_not_truncated"] = next(
        ((g + (w,), 3) for g in tri if brute.grams[g][1] != 0.0 and g[1:] in brute.grams
         for w in sorted(lexicon & set(brute.ids)) if g[1:] + (w,) not in brute.grams), None)
    return out


def test_mutations_are_seen(sctc):
    """each mistake the device could make changes the result of a listed case; "lm_on_hold" needs the
    Hold term, so its case ends with frames in which the extension by the space is cut and comes back"""
    from decoder import decoder_utils, ngram_lm, prefixTree
    chars, words = decoder_utils.load_chars(CHARS), decoder_utils.load_words(WORDS)
    lm = ngram_lm.NgramLM(ARPA4, 4)
    child, word = prefixTree.PrefixTree(chars, words, lm, specials=["[laughter]", "[noise]"]).flatten(35)
    brute = ngm.BruteLM(ARPA4, 4)
    cases = mutation_cases(brute)
    assert sorted(cases) == sorted(m for m in ngm.MUTATIONS if m != "lm_on_hold")
    for mut, (sent, order) in cases.items():
        sent = [w for w in sent if w != "<s>"]
        lp, syms = forced(chars, sent, tail=[{1: -0.3, 0: -1.2}], seed=len(mut))
        good, bad = ngm.BruteLM(ARPA4, order), ngm.BruteLM(ARPA4, order, mutate=mut)
        run = lambda b, m: ngm.decode(lp, child, word, b.prob_ids, lm.start, 1, order, beam=8, alpha=0.8, beta=0.37,
                                      nbest=2, mutate=m)
        want, got = run(good, None), run(bad, mut)
        assert sorted(h for h, _ in want) == [tuple(syms), tuple(syms) + (1,)], mut
        assert got != want, "%s goes unnoticed on %s" % (mut, " ".join(sent))
        ref = ngram_lm.NgramLM(ARPA4, order)
        assert run(ref_wrapper(ref), None) == want
    # the Hold term: P + space is a candidate in frame t (space has mass), not kept (beam 1), and a
    # candidate again in frame t + 1, where its Hold masses count without the LM term
    w = next(w for w in words if (w,) in brute.grams and len(w) >= 2)
    lp, syms = forced(chars, [w], tail=[{0: -0.1, 1: -3.0}, {0: -12.0, 1: -0.2}], seed=3)
    good = ngm.BruteLM(ARPA4, 3)
    a = ngm.decode(lp, child, word, good.prob_ids, lm.start, 1, 3, beam=1, alpha=0.8, beta=0.0, nbest=1)
    b = ngm.decode(lp, child, word, good.prob_ids, lm.start, 1, 3, beam=1, alpha=0.8, beta=0.0, nbest=1,
                   mutate="lm_on_hold")
    assert a[0][0] == tuple(syms) + (1,) and a != b


class ref_wrapper(object):
    """decoder.ngram_lm.NgramLM behind the model's P(history ids, word id)"""

    def __init__(self, lm):
        self.prob_ids = lm.prob


# ---- the C entry point and the Python surface ----------------------------------------------------

def test_create_ngram_argument_errors_need_no_gpu(sctc):
    L = sctc.lib()
    A, nodes = 4, 3
    child = np.full((nodes, A), -1, dtype=np.int32)
    child[0, 2], child[1, 3] = 1, 2
    word = np.array([-1, -1, 1], dtype=np.int32)
    ug = np.zeros(3, dtype=np.float32)
    keys = np.full(4, EMPTY, dtype=np.uint64)
    keys[1] = (3 << 32) | 2                                # the trigram (context 3 = some bigram, word 2)
    keys[2] = (0 << 32) | 1                                # the bigram with the id 3
    vals = np.zeros(4, dtype=np.float32)
    ids = np.array([-1, -1, 3, -1], dtype=np.int32)
    h = ctypes.c_void_p()

    def create(child=child, word=word, keys=keys, ids=ids, cap=4, contexts=1, order=3, start=0, n_words=3):
        return L.sctc_lexicon_create_ngram(child.ctypes.data, word.ctypes.data, nodes, A, 1, ug.ctypes.data,
                                           ug.ctypes.data, n_words, keys.ctypes.data, vals.ctypes.data,
                                           vals.ctypes.data, ids.ctypes.data, cap, contexts, order, start,
                                           ctypes.byref(h))
    assert create(order=1) == -1 and b"order" in L.sctc_last_error()
    assert create(order=6) == -1 and b"order" in L.sctc_last_error()
    assert create(cap=3) == -1 and b"power of two" in L.sctc_last_error()
    assert create(ids=np.array([-1, -1, 4, -1], dtype=np.int32)) == -1 and b"id" in L.sctc_last_error()
    assert create(ids=np.array([-1, -1, 1, -1], dtype=np.int32)) == -1      # a word's id is no n-gram's
    assert create(ids=np.array([-1, -2, 3, -1], dtype=np.int32)) == -1
    assert create(contexts=0) == -1                         # the context 3 of slot 1 is then outside the table
    # ids that do not fit the n-grams' lengths: the bigram without an id below full order, the trigram with one at
    # full order, an id two n-grams share, a context no listed n-gram has
    assert create(ids=np.array([-1, -1, -1, -1], dtype=np.int32)) == -1
    assert create(ids=np.array([-1, 4, 3, -1], dtype=np.int32), contexts=2) == -1 and b"order" in L.sctc_last_error()
    two = keys.copy()
    two[3] = (1 << 32) | 2
    assert create(keys=two, ids=np.array([-1, -1, 3, 3], dtype=np.int32)) == -1
    alone = keys.copy()
    alone[2] = EMPTY                                        # the trigram's context 3 is no listed n-gram's id
    assert create(keys=alone, ids=np.full(4, -1, dtype=np.int32)) == -1 and b"context" in L.sctc_last_error()
    bad = keys.copy()
    bad[1] = (3 << 32) | 3                                  # a word outside the vocabulary
    assert create(keys=bad) == -1
    full = np.array([1, 2, (1 << 32) | 1, (2 << 32) | 1], dtype=np.uint64)
    assert create(keys=full, ids=np.full(4, -1, dtype=np.int32)) == -1 and b"empty slot" in L.sctc_last_error()
    assert create(start=3) == -1 and create(start=-1) == -1
    assert create(word=np.array([-1, -1, 3], dtype=np.int32)) == -1         # a word id outside the vocabulary
    assert L.sctc_lexicon_create_ngram(None, word.ctypes.data, nodes, A, 1, ug.ctypes.data, ug.ctypes.data, 3,
                                       keys.ctypes.data, vals.ctypes.data, vals.ctypes.data, ids.ctypes.data, 4, 1, 3,
                                       0, ctypes.byref(h)) == -1
    assert h.value is None


def test_python_surface_rejects_before_the_device(sctc):
    import ctc_fast
    from decoder import decoder_utils, lm as lm_mod
    chars = decoder_utils.load_chars(CHARS)
    for order in (7, 1, 0):
        with pytest.raises(ValueError):
            ctc_fast.DecodeLexicon(["at"], chars, ARPA4, "[space]", order=order)
    with pytest.raises(ValueError):
        ctc_fast.DecodeLexicon(["at"], chars, ARPA4, "[space]", order=5)     # the file stops at 4-grams
    with pytest.raises(ValueError):
        ctc_fast.DecodeLexicon(["at"], chars, lm_mod.LM(ARPA), "[space]", order=3)
    from decoder import ngram_lm
    with pytest.raises(ValueError, match="order 4 asked"):
        ctc_fast.DecodeLexicon(["at"], chars, ngram_lm.NgramLM(ARPA4, 3), "[space]", order=4)
