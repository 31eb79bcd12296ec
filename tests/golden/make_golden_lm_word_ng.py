"""Writes tests/golden/lm_word_4g.arpa: a synthetic word 4-gram over words_bg.txt for the lexicon
decoder's n-gram LM.  Seeded, NumPy only; nothing of the package or of the
reference is used.

    python tests/golden/make_golden_lm_word_ng.py

What the file holds, and the tests rely on:
* <s>, </s>, <UNK>, [noise] and [laughter] first, then the lexicon's words in their order, 12 of them
  left out (they decode as <UNK>);
* unigrams, bigrams and trigrams with and without the back-off column (4-grams never have one);
* 25 listed n-grams of each order 2..4 whose value is exactly 0.000000;
* every listed n-gram's prefix is listed (a trigram extends a listed bigram, a 4-gram a listed
  trigram), but not every suffix: most trigrams a b c are drawn so that b c is listed too, at least
  30 so that it is not, and likewise for the 4-grams and b c d -- the shape of a pruned model;
* contexts that are missing, so that a back-off sum stops early, come with that;
* half of the n-grams stay within the first 60 words, the lexica the small cases use.
"""
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
NOT_IN_LM = 12
N2, N3, N4 = 1500, 1300, 800
ZEROS = 25


def main():
    rs = np.random.RandomState(4)
    words = [l.strip() for l in open(os.path.join(OUT, "words_bg.txt")) if l.strip()]
    out_of_lm = set(rs.choice(np.arange(5, len(words)), size=NOT_IN_LM, replace=False).tolist())
    vocab = ["<s>", "</s>", "<UNK>", "[noise]", "[laughter]"] + [w for i, w in enumerate(words) if i not in out_of_lm]
    V = len(vocab)

    def value():
        return -(0.1 + 3.0 * rs.rand())

    def backoff(p_none):
        return None if rs.rand() < p_none else -(0.05 + 1.5 * rs.rand())

    def word():
        return int(rs.randint(2, 62)) if rs.rand() < 0.5 else int(rs.randint(2, V))

    uni = [(-99.0 if w == "<s>" else -(1.0 + 3.0 * rs.rand()), None if w == "</s>" else backoff(0.15)) for w in vocab]
    grams = {2: {}, 3: {}, 4: {}}
    while len(grams[2]) < N2:
        a = 0 if rs.rand() < 0.08 else word()
        b = 1 if rs.rand() < 0.02 else word()
        grams[2][(a, b)] = [value(), None if b == 1 else backoff(0.2)]
    follow = {}                 # context -> the words that extend it to a listed n-gram
    for n, count in ((3, N3), (4, N4)):
        for g in grams[n - 1]:
            follow.setdefault(g[:-1], []).append(g[-1])
        prefixes = sorted(g for g in grams[n - 1] if g[-1] != 1)
        while len(grams[n]) < count:
            g = prefixes[rs.randint(len(prefixes))]
            nxt = follow.get(g[1:])
            if nxt and rs.rand() < 0.85:
                c = nxt[rs.randint(len(nxt))]             # the suffix is listed
            else:
                c = word()                                # it is not, most of the time
            grams[n][g + (c,)] = [value(), None if (n == 4 or c == 1) else backoff(0.2)]
    for n in (2, 3, 4):
        keys = sorted(grams[n])
        for i in rs.choice(len(keys), size=ZEROS, replace=False):
            grams[n][keys[i]][0] = 0.0
    for n in (3, 4):
        assert all(g[:-1] in grams[n - 1] for g in grams[n])
        open_suffix = sum(g[1:] not in grams[n - 1] for g in grams[n])
        print("%d-grams: %d, suffix not listed: %d" % (n, len(grams[n]), open_suffix))
        assert open_suffix >= 30

    lines = ["\\data\\", "ngram 1=%d" % V] + ["ngram %d=%d" % (n, len(grams[n])) for n in (2, 3, 4)]
    lines += ["", "\\1-grams:"]
    for (p, bo), w in zip(uni, vocab):
        lines.append("%.6f\t%s" % (p, w) + ("" if bo is None else "\t%.6f" % bo))
    for n in (2, 3, 4):
        lines += ["", "\\%d-grams:" % n]
        for g in sorted(grams[n]):
            p, bo = grams[n][g]
            lines.append("%.6f\t%s" % (p, " ".join(vocab[i] for i in g)) + ("" if bo is None else "\t%.6f" % bo))
    lines += ["", "\\end\\", ""]
    path = os.path.join(OUT, "lm_word_4g.arpa")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= 150 * 1024


if __name__ == "__main__":
    main()
