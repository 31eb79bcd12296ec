"""A word n-gram LM of order 2..5 for the lexicon decoder, read from an ARPA
file: ``NgramLM(arpafile, order=None)`` with ``order``, ``num_words``, ``start``, ``end``, ``unk``,
``get_word_id``, ``prob``, ``score`` and ``pack``.

* word ids are the order of the 1-gram section, an unknown word has the id of ``<UNK>`` / ``<unk>``
  (``ValueError`` with neither) and a stored value is float32 of ``(double)float32(ln 10) *
  atof(text)``: all as :class:`decoder.lm.LM`, so ``alpha`` means the same for both;
* ``order`` defaults to the file's highest section; sections above it are ignored, a request above
  the file's highest section is a ``ValueError``;
* ``prob(history, w)`` is the ARPA back-off rule of ``arpa_lm.ArpaLM.score_ids`` in kenlm's order
  of float32 additions: the value of the longest listed ``h' w``, the match extended one context
  word at a time and stopped at the first miss, plus the back-offs of the contexts from that length
  up to the whole history, shortest first, stopped at the first context that is not listed.  Unlike
  ``LM.bg_prob`` a listed value of exactly 0.0 is a value;
* the prefix ``w1 .. w(n-1)`` of every listed n-gram must be listed (ARPA writers guarantee it: a
  context needs a back-off weight); a file that breaks this is rejected with the n-gram.  The
  suffix ``w2 .. wn`` need not be: pruned models drop it, and "stopped at the first miss" comes out
  the same for them.

``pack()`` lays the model out for ``sctc_lexicon_create_ngram``; ``walk_packed`` is the host twin of
the device's walk through that table.
"""
import numpy as np

import arpa_lm
from decoder.lm import BG_EMPTY, _value

MIN_ORDER, MAX_ORDER = 2, 5


class NgramLM(object):
    def __init__(self, arpafile, order=None):
        if order is not None and not MIN_ORDER <= int(order) <= MAX_ORDER:
            raise ValueError("NgramLM: order %s outside %d..%d" % (order, MIN_ORDER, MAX_ORDER))
        self.word_to_int = {}
        ug, bo = [], []
        self.ngrams = {}              # (w1, .., wn), n >= 2 -> (value, back-off), in file order
        section, top = 0, 0
        want = int(order) if order is not None else MAX_ORDER
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
                    top = max(top, section)
                    continue
                if section == 1 and len(s) >= 2:
                    self.word_to_int[s[1]] = len(ug)
                    ug.append(_value(s[0]))
                    bo.append(_value(s[2]) if len(s) >= 3 else np.float32(0.0))
                elif 2 <= section <= want and len(s) >= section + 1:
                    words = s[1:section + 1]
                    try:
                        ids = tuple(self.word_to_int[w] for w in words)
                    except KeyError:
                        raise ValueError("NgramLM: n-gram '%s' names a word without a unigram" % " ".join(words))
                    if section > 2 and ids[:-1] not in self.ngrams:
                        raise ValueError("NgramLM: n-gram '%s' is listed, its prefix '%s' is not"
                                         % (" ".join(words), " ".join(words[:-1])))
                    self.ngrams[ids] = (_value(s[0]), _value(s[section + 1]) if len(s) >= section + 2
                                        else np.float32(0.0))
        if not ug:
            raise ValueError("NgramLM: %s has no 1-gram section" % arpafile)
        if order is None:
            order = min(top, MAX_ORDER)
        if top < int(order) or int(order) < MIN_ORDER:
            raise ValueError("NgramLM: order %d asked, the highest section of %s is %d" % (int(order), arpafile, top))
        self.order = int(order)
        self.ug = np.array(ug, dtype=np.float32)
        self.bo = np.array(bo, dtype=np.float32)
        self.num_words = len(ug)
        for name in ("<s>", "</s>"):
            if name not in self.word_to_int:
                raise ValueError("NgramLM: %s has no %s" % (arpafile, name))
        self.start = self.word_to_int["<s>"]
        self.end = self.word_to_int["</s>"]
        self.unk = self.word_to_int.get("<UNK>", self.word_to_int.get("<unk>"))

    def get_word_id(self, word):
        wid = self.word_to_int.get(word)
        if wid is not None:
            return wid
        if self.unk is None:
            raise ValueError("NgramLM: unknown word %r and the LM has no <UNK>" % (word,))
        return self.unk

    def _entry(self, ids):
        """(value, back-off) of a listed n-gram of any length, or None"""
        if len(ids) == 1:
            return self.ug[ids[0]], self.bo[ids[0]]
        return self.ngrams.get(ids)

    def prob(self, history_ids, w):
        """float32 P(w | history), history = word ids oldest first (``<s>`` included)"""
        ctx = tuple(int(h) for h in history_ids)[-(self.order - 1):]
        w = int(w)
        p, n = self.ug[w], 1
        for m in range(1, len(ctx) + 1):
            g = self.ngrams.get(ctx[len(ctx) - m:] + (w,))
            if g is None:
                break
            p, n = g[0], m + 1
        p = np.float32(p)
        for m in range(n, len(ctx) + 1):
            g = self._entry(ctx[len(ctx) - m:])
            if g is None:
                break
            p = np.float32(p + g[1])
        return p

    def score(self, sentence):
        """float32 running sum over <s> w1 .. wn, without a </s> term"""
        hist = [self.start]
        total = np.float32(0.0)
        for w in sentence.split():
            wid = self.get_word_id(w)
            total = np.float32(total + self.prob(hist, wid))
            hist.append(wid)
        return total

    def pack(self):
        """(keys uint64[cap], values float32[cap], back-offs float32[cap], ids int32[cap], contexts):
        every listed n-gram of length 2..order-1 gets a dense id after the word ids (num_words ..
        num_words + contexts - 1), a unigram's id is its word id.  One open-addressing table holds
        every listed n-gram w1..wn, n >= 2, under the key (id of w1..w(n-1) << 32) | wn: all ones =
        empty, slot = splitmix64(key) & (cap-1), linear probing, load <= 1/2.  A slot's id is the
        n-gram's own, -1 at full order."""
        ctx_id = {}
        for g in self.ngrams:
            if len(g) < self.order:
                ctx_id[g] = self.num_words + len(ctx_id)
        n = len(self.ngrams)
        cap = 2
        while cap < 2 * n + 2:
            cap *= 2
        keys = np.full(cap, BG_EMPTY, dtype=np.uint64)
        vals = np.zeros(cap, dtype=np.float32)
        bos = np.zeros(cap, dtype=np.float32)
        ids = np.full(cap, -1, dtype=np.int32)
        if n:
            grams = list(self.ngrams)
            k = np.array([((g[0] if len(g) == 2 else ctx_id[g[:-1]]) << 32) | g[-1] for g in grams], dtype=np.uint64)
            pos = (arpa_lm.mix64(k) & np.uint64(cap - 1)).astype(np.int64).tolist()
            used = [False] * cap
            slot = np.empty(n, dtype=np.int64)
            for i in range(n):
                s = pos[i]
                while used[s]:
                    s = (s + 1) & (cap - 1)
                used[s] = True
                slot[i] = s
            keys[slot] = k
            vals[slot] = np.array([self.ngrams[g][0] for g in grams], dtype=np.float32)
            bos[slot] = np.array([self.ngrams[g][1] for g in grams], dtype=np.float32)
            ids[slot] = np.array([ctx_id.get(g, -1) for g in grams], dtype=np.int32)
        return keys, vals, bos, ids, len(ctx_id)


def find_packed(table, ctx, w):
    """slot of the n-gram (context id, w) in a packed table, or -1"""
    keys = table[0]
    cap = keys.shape[0]
    key = (int(ctx) << 32) | int(w)
    s = int(arpa_lm.mix64(np.array([key], dtype=np.uint64))[0]) & (cap - 1)
    while True:
        k = int(keys[s])
        if k == key:
            return s
        if k == int(BG_EMPTY):
            return -1
        s = (s + 1) & (cap - 1)


def walk_packed(table, ug, bo, history_ids, w, order):
    """float32 P(w | history) from the arrays of ``pack`` alone, the way the device walks them
    (csrc/beam_policies.h ``lex_ng``): per context length m the id of the history's suffix of that
    length by chaining from its oldest word, then (context, w) while the match holds, the context's
    back-off after it"""
    _, vals, bos, ids, _ = table
    h = [int(x) for x in history_ids][-(order - 1):][::-1]          # newest first
    p = np.float32(ug[w])
    matching = True
    for m in range(1, len(h) + 1):
        cid, cbo = h[m - 1], np.float32(bo[h[m - 1]])
        listed = True
        for i in range(m - 2, -1, -1):
            s = find_packed(table, cid, h[i])
            if s < 0:
                listed = False
                break
            cid, cbo = int(ids[s]), bos[s]
        if not listed:
            break
        if matching:
            s = find_packed(table, cid, w)
            if s >= 0:
                p = np.float32(vals[s])
                continue
            matching = False
        p = np.float32(p + cbo)
    return p
