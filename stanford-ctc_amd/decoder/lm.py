"""The word-bigram LM of the reference's ``decoder/fastdecode/lm.cpp``, read from an ARPA
file: ``LM(arpafile)`` with ``start``, ``end``, ``unk``, ``get_word_id``, ``ug_prob``,
``bg_prob`` and ``score_bg``.

* word ids are the order of the 1-gram section;
* a stored value is float32 of ``(double)float32(ln 10) * atof(text)`` (lm.h:14, lm.cpp:79-108):
  unigram value, unigram back-off (0 when the column is absent) and bigram value;
* ``bg_prob(w1, w2)`` is the listed bigram value when that is non-zero, otherwise the float32
  sum ``backoff(w1) + unigram(w2)`` (lm.cpp:119-127).  A listed bigram of exactly 0.0 therefore
  counts as missing; the quirk is kept;
* sections of order 3 and above are ignored by this class: ``decoder.ngram_lm.NgramLM`` reads them
  (orders 2..5);
* an unknown word has the id of ``<UNK>`` (``<unk>`` is accepted too); without either it is a
  ``ValueError`` where the C++ would silently use id 0.
"""
import numpy as np

import arpa_lm

SCALE = np.float32(np.log(10.0))
BG_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _value(text):
    return np.float32(float(SCALE) * float(text))


class LM(object):
    def __init__(self, arpafile):
        self.word_to_int = {}
        ug, bo = [], []
        self.bg = {}
        section = 0
        with open(arpafile) as f:
            for line in f:
                s = line.split()
                if not s:
                    continue
                if s[0].startswith("\\"):
                    head = s[0]
                    if head == "\\end\\":
                        break
                    section = int(head[1:head.index("-")]) if head.endswith("-grams:") else 0
                    continue
                if section == 1 and len(s) >= 2:
                    self.word_to_int[s[1]] = len(ug)
                    ug.append(_value(s[0]))
                    bo.append(_value(s[2]) if len(s) >= 3 else np.float32(0.0))
                elif section == 2 and len(s) >= 3:
                    if s[1] not in self.word_to_int or s[2] not in self.word_to_int:
                        raise ValueError("LM: bigram '%s %s' names a word without a unigram" % (s[1], s[2]))
                    self.bg[(self.word_to_int[s[1]], self.word_to_int[s[2]])] = _value(s[0])
        if not ug:
            raise ValueError("LM: %s has no 1-gram section" % arpafile)
        self.ug = np.array(ug, dtype=np.float32)
        self.bo = np.array(bo, dtype=np.float32)
        self.num_words = len(ug)
        for name in ("<s>", "</s>"):
            if name not in self.word_to_int:
                raise ValueError("LM: %s has no %s" % (arpafile, name))
        self.start = self.word_to_int["<s>"]
        self.end = self.word_to_int["</s>"]
        self.unk = self.word_to_int.get("<UNK>", self.word_to_int.get("<unk>"))

    def get_word_id(self, word):
        wid = self.word_to_int.get(word)
        if wid is not None:
            return wid
        if self.unk is None:
            raise ValueError("LM: unknown word %r and the LM has no <UNK>" % (word,))
        return self.unk

    def ug_prob(self, wid):
        return self.ug[wid]

    def bg_prob(self, w1, w2):
        """float32, as lm.cpp:119-127"""
        p = self.bg.get((w1, w2), np.float32(0.0))
        if p == 0.0:
            p = np.float32(self.bo[w1] + self.ug[w2])
        return p

    def score_bg(self, sentence):
        """float32 running sum over <s> w1 .. wn </s> (lm.cpp:129-152)"""
        ids = [self.get_word_id(w) for w in sentence.split()]
        seq = [self.start] + ids + [self.end]
        score = np.float32(0.0)
        for a, b in zip(seq[:-1], seq[1:]):
            score = np.float32(score + self.bg_prob(a, b))
        return score

    def pack_bigrams(self):
        """(keys uint64[cap], values float32[cap]) for sctc_lexicon_create: open addressing, key
        (w1 << 32) | w2, all ones = empty, slot = splitmix64(key) & (cap-1), linear probing,
        load <= 1/2"""
        n = len(self.bg)
        cap = 2
        while cap < 2 * n + 2:
            cap *= 2
        keys = np.full(cap, BG_EMPTY, dtype=np.uint64)
        vals = np.zeros(cap, dtype=np.float32)
        if n:
            pairs = np.array(list(self.bg.keys()), dtype=np.uint64)
            k = (pairs[:, 0] << np.uint64(32)) | pairs[:, 1]
            v = np.array(list(self.bg.values()), dtype=np.float32)
            pos = (arpa_lm.mix64(k) & np.uint64(cap - 1)).astype(np.int64)
            for i in range(n):
                s = int(pos[i])
                while keys[s] != BG_EMPTY:
                    s = (s + 1) & (cap - 1)
                keys[s] = k[i]
                vals[s] = v[i]
        return keys, vals
