"""Python restatement of the lexicon-constrained word-bigram prefix beam search of DESIGN.md
§4.6 (the reference's ``decode_bg_lm``, ctc_fast/decoder/bg_decoder.pyx:18-95), written the way
the device kernel works.  It is ``beam_model.decode`` with four differences:

1. every prefix carries (node, prevId, numW), starting as (root, lm.start, 0);
2. P+c exists only when the tree allows it: c == space after a whole word (new state: root,
   the word's id, numW + 1), any other c along a child edge (new state: the child, prevId,
   numW); a forbidden extension is no candidate at all;
3. the LM term of an extension is alpha * bg_prob(prevId, node.id) for c == space and 0
   otherwise, a float64 product of a float32 value; it does not apply to the Hold term;
4. the sort key is log(p_nb + p_b) + beta * numW.

The tree is given flattened (``PrefixTree.flatten``): child[n, c] and word[n]; ``bg(w1, w2)``
returns the float32 bigram value.  Cell index = beam rank * A + symbol, as in beam_model."""
import numpy as np

from tests.beam_model import NEG, lse, f32


def decode(probs, child, word, bg, start, space, beam=40, alpha=1.0, beta=0.0, nbest=1, trace=None):
    """probs: (A, T) natural-log probabilities.  Returns [(prefix tuple, score)] of the best
    ``nbest`` (fewer when fewer prefixes are alive).  trace: a list that receives the whole new
    beam of every frame as [(prefix, key)]."""
    probs = np.asarray(probs, dtype=np.float64)
    A, T = probs.shape
    # beam: (prefix, p_nb f32, p_b f32, key f64); state: prefix -> (node, prevId, numW)
    cur = [((), NEG, 0.0, 0.0)]
    state = {(): (0, int(start), 0)}
    hold = {}
    allowed = {}
    for t in range(T):
        y = probs[:, t]
        idx = {p: j for j, (p, _, _, _) in enumerate(cur)}
        cells = []                 # (key, cell index, prefix, nb, b, state)
        for j, (P, v0, v1, _) in enumerate(cur):
            node, prev, numw = state[P]
            l = P[-1] if P else -1
            nb = [v0 + y[l]] if P else []
            if P and P[:-1] in idx:
                pj = idx[P[:-1]]
                _, w0, w1, _ = cur[pj]
                pnode, pprev, _ = state[P[:-1]]
                lm = alpha * float(bg(pprev, int(word[pnode]))) if l == space else 0.0
                if len(P) == 1 or P[-2] != l:
                    nb.append(w0 + y[l] + lm)
                nb.append(w1 + y[l] + lm)
            nbv = lse(*nb) if nb else NEG
            bv = lse(v0 + y[0], v1 + y[0])
            cells.append((lse(nbv, bv) + beta * numw, j * A, P, nbv, bv, state[P]))
            if node not in allowed:        # the symbols that may follow, ascending (space: -1 as the child)
                ext = [(int(c), int(child[node, c])) for c in np.nonzero(child[node] >= 0)[0] if c != space]
                if word[node] >= 0:
                    ext.append((space, -1))
                allowed[node] = sorted(ext)
            for c, nxt in allowed[node]:
                if c == space:
                    st = (0, int(word[node]), numw + 1)
                    lm = alpha * float(bg(prev, int(word[node])))
                else:
                    st = (nxt, prev, numw)
                    lm = 0.0
                Q = P + (c,)
                if Q in idx:
                    continue
                nb = [v1 + y[c] + lm]
                if c != l:
                    nb.append(v0 + y[c] + lm)
                h2, h3 = hold.get(Q, (NEG, NEG))
                nb.append(h2 + y[c])
                nbv = lse(*nb)
                bv = lse(h2 + y[0], h3 + y[0])
                cells.append((lse(nbv, bv) + beta * st[2], j * A + c, Q, nbv, bv, st))
        hold = {P: (f32(nbv), f32(bv)) for _, _, P, nbv, bv, _ in cells}
        cells.sort(key=lambda e: (-e[0], e[1]))
        cur = [(P, f32(nbv), f32(bv), key) for key, _, P, nbv, bv, _ in cells[:beam]]
        state = {P: st for _, _, P, _, _, st in cells[:beam]}
        if trace is not None:
            trace.append([(e[2], e[0]) for e in cells[:beam]])
    return [(P, key) for P, _, _, key in cur[:nbest]]


def from_objects(tree, lm, A):
    """(child, word, bg, start, space) of a decoder.prefixTree.PrefixTree and a decoder.lm.LM"""
    child, word = tree.flatten(A)
    return child, word, lm.bg_prob, lm.start, tree.space
