"""A restatement in plain Python / float64 of the n-best MBR contract (include/sctc.h): word
interning, the pairwise distances (through tests/edit_model.py), weights / risks / choice / order, and the confidences
from edit_model's paths.  The tests compare the device with this bit for bit where the arithmetic is exact and within a
derived bound where exp() is involved.

The keyword switches named ``mut_*`` each break one rule; tests/test_mbr_model_cpu.py shows that every one of them
changes a hand-worked case, so that a device that had the rule wrong could not pass against the model by accident."""
import functools
import math

import numpy as np

from tests import edit_model


@functools.lru_cache(maxsize=None)
def _edit_cached(a, b):
    stats, path = edit_model.edit_model(a, b)
    return int(stats[0]), tuple(int(o) for o in path)


def _edit(a, b):
    """(distance, path) of edit_model for a = rows, b = columns; n-best lists repeat their pairs"""
    return _edit_cached(tuple(int(x) for x in a), tuple(int(x) for x in b))


def tokens(row, space, mut_empty_words=False):
    """the words of a row as tuples of symbols: maximal runs of symbols other than the space"""
    out, cur = [], []
    for c in row:
        if c == space:
            if cur or mut_empty_words:      # the mutation is str.split(' '): every space ends a word, empty or not
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(int(c))
    if cur or (mut_empty_words and len(row)):
        out.append(tuple(cur))
    return out


def intern(rows, groups, space, A, mut_prefix=False, mut_empty_words=False):
    """(ids: list of int32 arrays, one per row; counts int32 [N]; status int32 [N]).  groups: [G + 1] row offsets.
    The id of a token is the number, within its group in (row, position) order, of the first token with the same
    symbols.  A row with a label outside [1, A) has status 2 and no words."""
    N = len(rows)
    ids = [None] * N
    counts = np.zeros(N, dtype=np.int32)
    status = np.zeros(N, dtype=np.int32)
    for g in range(len(groups) - 1):
        seen = []                   # (word, first token number)
        t = 0
        for n in range(groups[g], groups[g + 1]):
            row = [int(c) for c in rows[n]]
            if any(c < 1 or c >= A for c in row):
                status[n] = 2
                ids[n] = np.zeros(0, dtype=np.int32)
                continue
            got = []
            for w in tokens(row, space, mut_empty_words):
                rep = None
                for word, first in seen:
                    same = word[:len(w)] == w or w[:len(word)] == word if mut_prefix else word == w
                    if same:
                        rep = first
                        break
                if rep is None:
                    rep = t
                    seen.append((w, t))
                got.append(rep)
                t += 1
            ids[n] = np.array(got, dtype=np.int32)
            counts[n] = len(got)
    return ids, counts, status


def intern_buffers(rows, groups, space, A, fill=-77):
    """the device's flat buffers: word ids at the rows' slots (row n from sum ceil(U / 2) of the rows before), the
    slots that are not written left at `fill`"""
    ids, counts, status = intern(rows, groups, space, A)
    per = [(len(r) + 1) // 2 for r in rows]
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    flat = np.full(int(first[-1]), fill, dtype=np.int32)
    for n, v in enumerate(ids):
        flat[first[n]:first[n] + len(v)] = v
    return flat, counts, status, first


def mbr(hyps, scores, unit="word", scale=1.0, space=None, A=256, order=None, K_b=None, confidences=False,
        mut_tie=False, mut_descending=False, mut_normalise_first=False, mut_conf_other=False, mut_prefix=False,
        mut_empty_words=False):
    """hyps: B lists of K label rows; scores [B][K].  Returns a dict: best int32 [B], posterior / risk float64 [B, K],
    order int32 [B, K], dist int32 [B, K, K], and with ``confidences`` confidence (a list of float64 arrays) and
    conf_len int32 [B]."""
    B = len(hyps)
    K = len(hyps[0]) if B else 1
    scores = np.asarray(scores, dtype=np.float64).reshape(B, K)
    best = np.full(B, -1, dtype=np.int32)
    post = np.zeros((B, K), dtype=np.float64)
    risk = np.full((B, K), np.inf, dtype=np.float64)
    out_order = np.zeros((B, K), dtype=np.int32)
    dist = np.full((B, K, K), -1, dtype=np.int32)
    conf, conf_len = [], np.zeros(B, dtype=np.int32)
    for b in range(B):
        kb = K if K_b is None else int(K_b[b])
        real = [k < kb and math.isfinite(scores[b, k]) for k in range(K)]
        if unit == "word":
            rows = [list(hyps[b][k]) if k < kb else [] for k in range(K)]
            u, _, _ = intern(rows, [0, K], space, A, mut_prefix=mut_prefix, mut_empty_words=mut_empty_words)
        else:
            u = [np.asarray(hyps[b][k], dtype=np.int32).reshape(-1) for k in range(K)]
        rk = [k for k in range(K) if real[k]]
        for k in rk:
            dist[b, k, k] = 0
            for j in rk:
                if k < j:
                    dist[b, k, j] = dist[b, j, k] = _edit(u[k], u[j])[0]
        pos = list(range(K))
        if order is not None and not mut_tie:
            for i, o in enumerate(order[b]):
                pos[int(o)] = i
        if rk:
            s_max = max(scores[b, k] for k in rk)
            w = [0.0] * K
            for k in rk:
                w[k] = 1.0 if scores[b, k] == s_max else math.exp(scale * (scores[b, k] - s_max))
            Z = 0.0
            for k in rk:
                Z += w[k]
            js = rk[::-1] if mut_descending else rk
            for k in rk:
                post[b, k] = w[k] / Z
                acc = 0.0
                for j in js:
                    acc += (w[j] / Z if mut_normalise_first else w[j]) * float(dist[b, k, j])
                risk[b, k] = acc if mut_normalise_first else acc / Z
            ranked = sorted(rk, key=lambda k: (risk[b, k], pos[k], k))
            best[b] = ranked[0]
        else:
            ranked = []
        out_order[b] = ranked + [k for k in range(K) if not real[k]]
        if confidences:
            c = int(best[b])
            if c < 0:
                conf.append(np.zeros(0, dtype=np.float64))
                continue
            n = len(u[c])
            conf_len[b] = n
            acc = [0.0] * n
            for j in rk:
                if j == c:
                    match = [1] * n
                elif mut_conf_other:
                    path = _edit(u[j], u[c])[1]      # the chosen hypothesis on the b side
                    match = [int(o == edit_model.MATCH) for o in path if o != edit_model.UP]
                else:
                    path = _edit(u[c], u[j])[1]
                    match = [int(o == edit_model.MATCH) for o in path if o != edit_model.LEFT]
                assert len(match) == n
                for i in range(n):
                    acc[i] += w[j] * float(match[i])
            conf.append(np.array([a / Z for a in acc], dtype=np.float64))
    res = {"best": best, "posterior": post, "risk": risk, "order": out_order, "dist": dist}
    if confidences:
        res["confidence"] = conf
        res["conf_len"] = conf_len
    return res


def min_risk_gap(res):
    """smallest relative gap between neighbouring finite risks of any utterance (inf when there is none): the general
    tests compare `best` and `order` only where it is clearly above the arithmetic's noise"""
    gap = np.inf
    for b in range(res["risk"].shape[0]):
        r = np.sort(res["risk"][b][np.isfinite(res["risk"][b])])
        for x, y in zip(r, r[1:]):
            gap = min(gap, (y - x) / max(abs(y), 1e-300))
    return gap
