"""Python restatement of the lexicon-constrained prefix beam search with a word n-gram LM (DESIGN.md
§4.6b).  It is ``lex_beam_model.decode`` with an opaque history in place of ``prevId``:

1. every prefix carries (node, history, numW), starting as (root, (<s>,), 0); the history is the tuple
   of the last min(order - 1, finished words + 1) word ids, oldest first;
2. emitting the space after a word w: history <- (history + (w,))[-(order - 1):], node <- root,
   numW + 1;
3. the LM term of that extension is alpha * P(w | history), a float64 product of a float32 value; it
   does not apply to the Hold term.

``P(history, w)`` is any callable; ``BruteLM`` is the ARPA back-off rule on tuples of strings, parsed
from the ARPA text here and sharing nothing with decoder/ngram_lm.py.

``mutate`` names one deliberate mistake, for the tests that show which cases would notice it:
MUTATIONS lists them."""
import numpy as np

from tests.beam_model import NEG, lse, f32

SCALE = float(np.float32(np.log(10.0)))
MUTATIONS = ("no_stop_at_first_miss", "backoffs_longest_first", "history_not_truncated", "lm_on_hold")


def val(text):
    return np.float32(SCALE * float(text))


class BruteLM(object):
    """the listed n-grams of an ARPA text as {tuple of words: (float32 value, float32 back-off)} and the
    back-off rule written out over them"""

    def __init__(self, path, order, mutate=None):
        self.order, self.mutate = order, mutate
        self.grams, self.words = {}, []
        sec = 0
        for line in open(path):
            s = line.split()
            if not s:
                continue
            if s[0].startswith("\\"):
                sec = int(s[0][1:s[0].index("-")]) if s[0].endswith("-grams:") else 0
            elif 1 <= sec <= order:
                g = tuple(s[1:sec + 1])
                self.grams[g] = (val(s[0]), val(s[sec + 1]) if len(s) > sec + 1 else np.float32(0.0))
                if sec == 1:
                    self.words.append(s[1])
        self.ids = {w: i for i, w in enumerate(self.words)}
        self.unk = "<UNK>" if "<UNK>" in self.ids else "<unk>"

    def name(self, wid):
        return self.words[wid]

    def prob(self, history, w):
        """history: words oldest first, w: a word; float32"""
        h = tuple(history)
        if self.mutate != "history_not_truncated":
            h = h[-(self.order - 1):]
        matched = 0                                    # context words of the longest listed h' w
        p = self.grams[(w,)][0]
        for m in range(1, len(h) + 1):
            g = self.grams.get(h[len(h) - m:] + (w,))
            if g is None:
                if self.mutate == "no_stop_at_first_miss":
                    continue
                break
            p, matched = g[0], m
        p = np.float32(p)
        terms = []
        for m in range(matched + 1, len(h) + 1):
            g = self.grams.get(h[len(h) - m:])
            if g is None:
                break
            terms.append(g[1])
        if self.mutate == "backoffs_longest_first":
            terms.reverse()
        for t in terms:
            p = np.float32(p + t)
        return p

    def prob_ids(self, history_ids, wid):
        return self.prob([self.words[i] for i in history_ids], self.words[wid])


def decode(probs, child, word, P, start, space, order, beam=40, alpha=1.0, beta=0.0, nbest=1, trace=None,
           mutate=None):
    """probs: (A, T) natural-log probabilities; P(history ids, word id) -> float32; start: the id of
    <s>.  Returns [(prefix tuple, score)] of the best ``nbest`` (fewer when fewer prefixes are alive)."""
    probs = np.asarray(probs, dtype=np.float64)
    A, T = probs.shape
    keep = order - 1 if mutate != "history_not_truncated" else 1 << 30
    cur = [((), NEG, 0.0, 0.0)]
    state = {(): (0, (int(start),), 0)}
    hold = {}
    allowed = {}
    memo = {}

    def term(hist, w):
        if (hist, w) not in memo:
            memo[(hist, w)] = alpha * float(P(hist, w))
        return memo[(hist, w)]

    for t in range(T):
        y = probs[:, t]
        idx = {p: j for j, (p, _, _, _) in enumerate(cur)}
        cells = []
        for j, (Pfx, v0, v1, _) in enumerate(cur):
            node, hist, numw = state[Pfx]
            l = Pfx[-1] if Pfx else -1
            nb = [v0 + y[l]] if Pfx else []
            if Pfx and Pfx[:-1] in idx:
                pj = idx[Pfx[:-1]]
                _, w0, w1, _ = cur[pj]
                pnode, phist, _ = state[Pfx[:-1]]
                lm = term(phist, int(word[pnode])) if l == space else 0.0
                if len(Pfx) == 1 or Pfx[-2] != l:
                    nb.append(w0 + y[l] + lm)
                nb.append(w1 + y[l] + lm)
            nbv = lse(*nb) if nb else NEG
            bv = lse(v0 + y[0], v1 + y[0])
            cells.append((lse(nbv, bv) + beta * numw, j * A, Pfx, nbv, bv, state[Pfx]))
            if node not in allowed:
                ext = [(int(c), int(child[node, c])) for c in np.nonzero(child[node] >= 0)[0] if c != space]
                if word[node] >= 0:
                    ext.append((space, -1))
                allowed[node] = sorted(ext)
            for c, nxt in allowed[node]:
                if c == space:
                    st = (0, (hist + (int(word[node]),))[-keep:], numw + 1)
                    lm = term(hist, int(word[node]))
                else:
                    st = (nxt, hist, numw)
                    lm = 0.0
                Q = Pfx + (c,)
                if Q in idx:
                    continue
                nb = [v1 + y[c] + lm]
                if c != l:
                    nb.append(v0 + y[c] + lm)
                h2, h3 = hold.get(Q, (NEG, NEG))
                nb.append(h2 + y[c] + (lm if mutate == "lm_on_hold" else 0.0))
                nbv = lse(*nb)
                bv = lse(h2 + y[0], h3 + y[0])
                cells.append((lse(nbv, bv) + beta * st[2], j * A + c, Q, nbv, bv, st))
        hold = {Q: (f32(nbv), f32(bv)) for _, _, Q, nbv, bv, _ in cells}
        cells.sort(key=lambda e: (-e[0], e[1]))
        cur = [(Q, f32(nbv), f32(bv), key) for key, _, Q, nbv, bv, _ in cells[:beam]]
        state = {Q: st for _, _, Q, _, _, st in cells[:beam]}
        if trace is not None:
            trace.append([(e[2], e[0]) for e in cells[:beam]])
    return [(Q, key) for Q, _, _, key in cur[:nbest]]
