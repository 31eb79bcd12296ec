#!/usr/bin/env python3
"""Generate the word-bigram beam search fixtures under tests/golden/ from the REFERENCE'S OWN
decoder.

The unmodified ``ctc_fast/decoder/bg_decoder.pyx`` of the reference checkout is cythonized
(language_level=2) in a scratch directory OUTSIDE the repository and runs under Python 3 with a
``collections`` shim whose ``defaultdict`` has ``iteritems`` (bg_decoder.pyx:93), assigned as
``bg_decoder.collections``.  It is fed tree and LM objects of this script's own:

* ``RefTree`` follows the reference's ``decoder/prefixTree.py:28-73``: ``root``, ``space``, nodes
  with ``isPrefix`` / ``isWord`` / ``children`` / ``id``, specials hanging off the root;
* ``RefLM`` follows ``decoder/fastdecode/lm.cpp:61-127`` (the reference's Python ``LM`` class is
  not in its tree): ids in 1-gram order, float32 of ``(double)float32(ln 10) * atof(text)``,
  ``bg_prob`` = the listed bigram unless that is 0, then the float32 sum back-off + unigram.
  The LM terms of the fixtures are therefore pinned to lm.cpp's formula.

Neither uses the project's ``decoder`` package, so the fixtures do not depend on the code they test.

Fixtures written:
  words_bg.txt        the word list: the first N_SMALL_ALPHA words use the letters of symbols 2..7
                      only (for the A = 8 cases); "small" lexica are the first N_SMALL words
  lm_word_2g.arpa     a synthetic word bigram with <s>, </s>, <UNK>; some lexicon words have no
                      unigram (-> <UNK>), some unigrams no back-off column, some words no bigram at
                      all, and some listed bigrams are exactly 0.000000 (lm.cpp treats them as missing)
  decode_bg_ref.npz   per case: inputs, configuration, the reference's hypothesis (symbol ids) and
                      score, and the top-2 key margin of the final beam from tests/lex_beam_model.py
                      (the reference returns only the top entry); hypotheses are compared only where
                      the margin is >= 1e-6 (at most 5 % of the cases may fall below), scores always

Usage:  python tests/golden/make_golden_decode_bg.py --reference <reference checkout> [--scratch DIR]
                                                     [--out DIR]
"""
import argparse
import collections as _collections
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import lex_beam_model  # noqa: E402

SPACE = "[space]"
N_SMALL_ALPHA = 120      # words 0..119 are spelled with a e t o n only
N_SMALL = 40
N_WORDS = 360
NOT_IN_LM = 12           # lexicon words without a unigram


class _DefaultDict(_collections.defaultdict):
    def iteritems(self):
        return iter(self.items())


class _CollectionsShim(object):
    defaultdict = _DefaultDict


def build_reference(ref, scratch):
    os.makedirs(scratch, exist_ok=True)
    pyx = os.path.join(ref, "ctc_fast/decoder/bg_decoder.pyx")
    setup = os.path.join(scratch, "setup_bg_decoder.py")
    with open(setup, "w") as f:
        f.write(
            "from setuptools import setup, Extension\n"
            "from Cython.Build import cythonize\n"
            "import numpy as np\n"
            "setup(ext_modules=cythonize([Extension('bg_decoder', [%r],\n"
            "      include_dirs=[np.get_include()])], language_level=2, build_dir=%r))\n"
            % (pyx, os.path.join(scratch, "cy_bg")))
    if not any(n.startswith("bg_decoder.") and n.endswith(".so") for n in os.listdir(scratch)):
        subprocess.check_call([sys.executable, setup, "build_ext", "--build-lib", scratch,
                               "--build-temp", os.path.join(scratch, "tmp_bg")], cwd=scratch,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, scratch)
    import bg_decoder  # noqa: the reference's Cython module
    bg_decoder.collections = _CollectionsShim
    return bg_decoder


# ---- stand-ins for the reference's tree and LM objects ---------------------------------------

class RefLM(object):
    """fastdecode/lm.cpp on an ARPA file"""

    def __init__(self, path):
        scale = float(np.float32(np.log(10.0)))
        self.ids, self.ug, self.bg = {}, [], {}
        sec = 0
        for line in open(path):
            s = line.split()
            if not s:
                continue
            if s[0] in ("\\1-grams:", "\\2-grams:"):
                sec = int(s[0][1])
            elif s[0].startswith("\\"):
                sec = 0
            elif sec == 1:
                self.ids[s[1]] = len(self.ug)
                self.ug.append((np.float32(scale * float(s[0])),
                                np.float32(scale * float(s[2])) if len(s) == 3 else np.float32(0.0)))
            elif sec == 2:
                self.bg[(self.ids[s[1]], self.ids[s[2]])] = np.float32(scale * float(s[0]))
        self.start, self.end, self.unk = self.ids["<s>"], self.ids["</s>"], self.ids["<UNK>"]

    def get_word_id(self, w):
        return self.ids.get(w, self.unk)

    def bg_prob(self, w1, w2):
        p = self.bg.get((w1, w2), np.float32(0.0))
        if p == 0.0:
            p = np.float32(p + np.float32(self.ug[w1][1] + self.ug[w2][0]))
        return float(p)


class RefNode(object):
    def __init__(self):
        self.isPrefix = False
        self.isWord = False
        self.children = None


class RefTree(object):
    """decoder/prefixTree.py:34-73 with the word list, specials and space as arguments"""

    def __init__(self, chars, words, lm, specials):
        self.root = RefNode()
        self.root.isPrefix = True
        self.space = chars[SPACE]
        self.root.children = _collections.defaultdict(RefNode)
        for w in specials:
            node = self.root.children[chars[w]]
            node.isWord = True
            node.id = lm.get_word_id(w)
        for w in words:
            node = self.root
            for k, ch in enumerate(w):
                if node.children is None:
                    node.children = _collections.defaultdict(RefNode)
                node = node.children[chars[ch]]
                if k == len(w) - 1:
                    node.isWord = True
                    node.id = lm.get_word_id(w)
                else:
                    node.isPrefix = True

    def flatten(self, A):
        order, number, i = [self.root], {id(self.root): 0}, 0
        while i < len(order):
            node = order[i]
            i += 1
            for sym in sorted(node.children or ()):
                ch = node.children[sym]
                if ch.isWord or ch.isPrefix:        # the reference's own look-ups leave empty nodes behind
                    number[id(ch)] = len(order)
                    order.append(ch)
        child = np.full((len(order), A), -1, dtype=np.int32)
        word = np.full(len(order), -1, dtype=np.int32)
        for n, node in enumerate(order):
            if node.isWord:
                word[n] = node.id
            for sym, ch in (node.children or {}).items():
                if id(ch) in number:
                    child[n, sym] = number[id(ch)]
        return child, word


# ---- the committed word list and LM -------------------------------------------------------------

def make_words(rs):
    small = list("aeton")
    full = list("aetonishrdlucmwfgypbvk'jxqz-.")
    words, seen = [], set()
    while len(words) < N_WORDS:
        letters = small if len(words) < N_SMALL_ALPHA else full
        w = "".join(rs.choice(letters, size=rs.randint(1, 7 if letters is full else 6)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words


def make_arpa(rs, words):
    out_of_lm = set(rs.choice(np.arange(5, N_WORDS), size=NOT_IN_LM, replace=False).tolist())
    vocab = ["<s>", "</s>", "<UNK>", "[noise]", "[laughter]"] + [w for i, w in enumerate(words) if i not in out_of_lm]
    uni = []
    for w in vocab:
        p = -99.0 if w == "<s>" else -(1.0 + 3.0 * rs.rand())
        bo = None if (w == "</s>" or rs.rand() < 0.15) else -(0.05 + 1.5 * rs.rand())
        uni.append((p, w, bo))
    no_bigram = set(rs.choice(np.arange(5, len(vocab)), size=40, replace=False).tolist())
    pairs = {}
    live = [i for i in range(2, len(vocab)) if i not in no_bigram]
    for i in live[:200]:                                  # sentence starts
        if rs.rand() < 0.6:
            pairs[(0, i)] = -(0.2 + 2.5 * rs.rand())
    while len(pairs) < 2600:
        a, b = live[rs.randint(len(live))], live[rs.randint(len(live))]
        if rs.rand() < 0.5:                               # favour the small lexica, which the cases visit most
            a, b = live[rs.randint(60)], live[rs.randint(60)]
        pairs[(a, b)] = -(0.1 + 3.0 * rs.rand())
    keys = sorted(pairs)
    for k in [keys[i] for i in rs.choice(len(keys), size=60, replace=False)]:
        pairs[k] = 0.0                                    # listed, exactly 0.000000: lm.cpp backs off
    lines = ["\\data\\", "ngram 1=%d" % len(uni), "ngram 2=%d" % len(pairs), "", "\\1-grams:"]
    for p, w, bo in uni:
        lines.append("%.6f\t%s" % (p, w) + ("" if bo is None else "\t%.6f" % bo))
    lines += ["", "\\2-grams:"]
    for (a, b) in keys:
        lines.append("%.6f\t%s %s" % (pairs[(a, b)], vocab[a], vocab[b]))
    lines += ["", "\\end\\", ""]
    return "\n".join(lines)


# ---- cases ---------------------------------------------------------------------------------------

def logsoftmax(x):
    m = x.max(axis=0, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))


def word_path(rs, chars, lexicon, specials, T):
    """frame labels of a random word sequence: runs of 1..3 frames per letter, blanks between equal
    neighbours and now and then elsewhere, a space between words"""
    path = []
    while len(path) < T:
        if specials and rs.rand() < 0.1:
            syms = [chars[specials[rs.randint(len(specials))]]]
        else:
            syms = [chars[ch] for ch in lexicon[rs.randint(len(lexicon))]]
        syms.append(chars[SPACE])
        for s in syms:
            if (path and path[-1] == s) or rs.rand() < 0.25:
                path += [0] * rs.randint(1, 3)
            path += [s] * rs.randint(1, 4)
    return path[:T]


def posteriors(rs, A, T, kind, chars, lexicon, specials):
    if kind == "flat":
        return logsoftmax(0.4 * rs.randn(A, T))
    x = 1.5 * rs.randn(A, T)
    path = np.array(word_path(rs, chars, lexicon, specials, T))
    x[path, np.arange(T)] += 6.0
    lp = logsoftmax(x)
    if kind == "neginf":
        mask = rs.rand(A, T) < 0.15
        mask[path, np.arange(T)] = False
        mask[0, :] = False
        lp[mask] = -np.inf
    return lp


CASES = [   # (A, T, beam, alpha, beta, lexicon, kind)
    (35, 1, 16, 0.8, 0.0, "small", "peaked"),
    (35, 2, 16, 1.3, 1.5, "large", "peaked"),
    (8, 1, 40, 1.3, 0.37, "small", "flat"),
    (8, 2, 1, 0.0, 0.0, "large", "peaked"),
    (8, 5, 1, 0.0, 0.0, "small", "peaked"),
    (8, 12, 16, 0.8, 0.0, "small", "flat"),
    (8, 40, 150, 1.3, 1.5, "large", "flat"),
    (8, 300, 1, 0.8, 1.5, "large", "peaked"),
    (8, 300, 16, 1.3, 0.37, "small", "peaked"),
    (8, 60, 40, 0.0, 0.37, "large", "peaked"),
    (8, 30, 16, 0.8, 0.0, "small", "neginf"),
    (8, 100, 40, 0.8, 1.5, "large", "neginf"),
    (8, 50, 150, 1.3, 0.0, "small", "peaked"),
    (8, 25, 150, 0.0, 1.5, "large", "flat"),
    (33, 20, 1, 0.0, 0.0, "small", "flat"),
    (33, 60, 16, 0.8, 0.0, "small", "peaked"),
    (33, 120, 16, 1.3, 1.5, "large", "peaked"),
    (33, 90, 1, 1.3, 0.0, "large", "peaked"),
    (33, 25, 150, 0.8, 0.37, "large", "peaked"),
    (33, 30, 16, 0.0, 1.5, "small", "neginf"),
    (33, 40, 40, 0.8, 1.5, "large", "neginf"),
    (33, 15, 150, 1.3, 0.0, "small", "flat"),
    (33, 300, 16, 0.8, 0.37, "large", "peaked"),
    (33, 45, 40, 1.3, 0.37, "small", "peaked"),
    (34, 50, 40, 0.8, 0.0, "large", "peaked"),
    (34, 30, 16, 1.3, 1.5, "small", "flat"),
    (35, 10, 16, 0.8, 0.0, "large", "flat"),
    (35, 30, 150, 0.0, 0.0, "small", "peaked"),
    (35, 40, 150, 0.8, 1.5, "large", "peaked"),
    (35, 20, 150, 1.3, 0.0, "large", "flat"),
    (35, 100, 1, 0.8, 0.37, "large", "peaked"),
    (35, 150, 16, 1.3, 1.5, "small", "peaked"),
    (35, 300, 40, 0.0, 0.37, "large", "peaked"),
    (35, 120, 1, 1.3, 1.5, "small", "peaked"),
    (35, 40, 16, 1.3, 0.0, "large", "neginf"),
    (35, 35, 150, 0.8, 1.5, "small", "neginf"),
    (35, 80, 16, 0.0, 1.5, "large", "flat"),
    (35, 200, 16, 0.8, 1.5, "large", "peaked"),
    (35, 45, 40, 1.3, 0.0, "large", "peaked"),
    (35, 45, 40, 0.8, 0.37, "small", "flat"),
    (35, 70, 40, 0.8, 0.0, "small", "peaked"),
    (35, 60, 40, 1.3, 0.37, "large", "neginf"),
]


def lexicon_of(words, A, size):
    """(words, specials) of a case"""
    if A == 8:
        return words[:N_SMALL if size == "small" else N_SMALL_ALPHA], ["[laughter]"]
    sp = ["[laughter]", "[noise]"] + (["[vocalized-noise]"] if A >= 34 else [])
    return words[:N_SMALL if size == "small" else N_WORDS], sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--scratch", default="/tmp/sctc_ref_bg_decoder")
    ap.add_argument("--out", default=HERE, help="where the fixtures are written")
    a = ap.parse_args()
    assert not os.path.abspath(a.scratch).startswith(ROOT), "scratch must be outside the repo"
    OUT = os.path.abspath(a.out)
    os.makedirs(OUT, exist_ok=True)
    rs = np.random.RandomState(2025)
    words = make_words(rs)
    with open(os.path.join(OUT, "words_bg.txt"), "w") as f:
        f.write("\n".join(words) + "\n")
    arpa = os.path.join(OUT, "lm_word_2g.arpa")
    with open(arpa, "w") as f:
        f.write(make_arpa(rs, words))
    chars = {}
    for l in open(os.path.join(HERE, "chars.txt")):
        tok, i = l.split()
        chars[tok] = int(i)
    dec = build_reference(a.reference, a.scratch)
    old_err = np.geterr()                     # bg_decoder.pyx:6 sets every numpy error to 'raise'
    np.seterr(all="ignore")
    lm = RefLM(arpa)
    assert any(v == 0.0 for v in lm.bg.values())
    trees = {}
    out = {"n": np.int64(len(CASES))}
    close = 0
    for i, (A, T, beam, alpha, beta, size, kind) in enumerate(CASES):
        assert alpha == 0.0 or float(np.float32(alpha)) != alpha
        lex, specials = lexicon_of(words, A, size)
        if (A, size) not in trees:
            trees[(A, size)] = RefTree(chars, lex, lm, specials)
        tree = trees[(A, size)]
        lp = np.asfortranarray(posteriors(rs, A, T, kind, chars, lex, specials))
        t0 = time.time()
        hyp, score = dec.decode_bg_lm(lp, tree, lm, beam, alpha, beta)
        dt = time.time() - t0
        child, word = tree.flatten(A)
        top2 = lex_beam_model.decode(lp, child, word, lm.bg_prob, lm.start, tree.space, beam, alpha, beta, nbest=2)
        margin = top2[0][1] - top2[1][1] if len(top2) > 1 else np.inf
        agree = list(top2[0][0]) == list(hyp)
        print("case %2d A=%2d T=%3d beam=%3d alpha=%.1f beta=%.2f %-5s %-7s score %.6f margin %.3g model %s "
              "(score diff %.2g) %.1fs" % (i, A, T, beam, alpha, beta, size, kind, score, margin,
                                           "agrees" if agree else "DIFFERS", abs(top2[0][1] - score), dt))
        assert np.isfinite(score) and score > -700, score
        close += margin < 1e-6
        out["lp%d" % i] = lp
        out["cfg%d" % i] = np.array([A, T, beam, alpha, beta], dtype=np.float64)
        out["lex%d" % i] = np.array(size)
        out["kind%d" % i] = np.array(kind)
        out["hyp%d" % i] = np.array(hyp, dtype=np.int32)
        out["score%d" % i] = np.float64(score)
        out["margin%d" % i] = np.float64(margin)
    assert close <= 0.05 * len(CASES), "%d cases with a top-2 margin below 1e-6: change seeds" % close
    np.savez_compressed(os.path.join(OUT, "decode_bg_ref.npz"), **out)
    np.seterr(**old_err)


if __name__ == "__main__":
    main()
