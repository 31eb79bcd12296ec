"""Float64 restatement of the recurrent character LM of DESIGN.md §4.10 (nn_lm.RNNCharLM), the
yardstick of the recurrent-LM decoder tests: the recurrence written as matrix products over an
explicit one-hot input, and the log10 softmax.  ``rows64(lm, sym_words)`` is an ``lm_row(prefix)``
provider for the unmodified tests/beam_model.decode and beam_trace.model_trace.

``forward32`` is the float32 evaluation that accumulates every sum in ascending k: the distance
d32 = max |forward32 - float64| over a set of prefixes is what float32 arithmetic of this model
costs, and the device may deviate from float64 by at most twice that.  Every test model has a
``Wh`` of spectral norm below 1 (``spectral_norm``), so that an error of the state does not grow
with the length of the prefix."""
import numpy as np

LOG10E = 0.43429448190325182765


def one_hot(lm, i, dtype=np.float64):
    x = np.zeros(lm.V, dtype=dtype)
    x[int(i)] = 1.0
    return x


def log10_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))) * LOG10E


def step64(lm, h, i, Wx=None, Wh=None, bh=None):
    """h' of the state h (None: no state, the zero vector) and the LM id i, with the input formed"""
    Wx = lm.Wx if Wx is None else Wx
    Wh = lm.Wh if Wh is None else Wh
    bh = lm.bh if bh is None else bh
    if h is None:
        h = np.zeros(Wh.shape[1])
    return np.maximum(bh.astype(np.float64) + Wx.astype(np.float64) @ one_hot(lm, i) + Wh.astype(np.float64) @ h, 0.0)


def state64(lm, ids, **kw):
    """the state of the prefix with LM ids ``ids``: <s> into no state, then one symbol at a time"""
    h = step64(lm, None, lm.bos, **kw)
    for i in ids:
        h = step64(lm, h, i, **kw)
    return h


def row64(lm, h, Wo=None):
    Wo = lm.Wo if Wo is None else Wo
    return log10_softmax(Wo.astype(np.float64) @ h + lm.bo.astype(np.float64))


def forward64(lm, ids):
    """(state, float64 log10 softmax row [V]) of a prefix of LM ids"""
    h = state64(lm, ids)
    return h, row64(lm, h)


def forward64_many(lm, prefixes):
    """(states [n, H], rows [n, V]) in float64 of prefixes of LM ids; the state of every prefix of
    a prefix is computed once"""
    states = {(): step64(lm, None, lm.bos)}
    out_s, out_r = [], []
    for P in prefixes:
        P = tuple(int(i) for i in P)
        for d in range(1, len(P) + 1):
            if P[:d] not in states:
                states[P[:d]] = step64(lm, states[P[:d - 1]], P[d - 1])
        out_s.append(states[P])
        out_r.append(row64(lm, states[P]))
    return np.stack(out_s), np.stack(out_r)


def matvec32(W, b, H):
    """b + W h for every row h of H [n, k], float32, accumulated in ascending k (one rounded multiply
    and one rounded add per term); b is one start vector for all rows or [n, units], one per row"""
    acc = np.array(np.broadcast_to(b.astype(np.float32), (H.shape[0], W.shape[0])))
    for k in range(W.shape[1]):
        acc = (acc + (H[:, k:k + 1] * W[:, k][None, :]).astype(np.float32)).astype(np.float32)
    return acc


def forward32(lm, prefixes):
    """(states float32 [n, H], rows float64 [n, V]) of prefixes of LM ids: float32 parameters and
    accumulation in ascending k, the accumulator of the recurrent layer starting from bh + Wx[:, id];
    the log-softmax in float64.  Every distinct prefix, and every prefix of it, is evaluated once,
    the prefixes of one depth together."""
    prefixes = [tuple(int(i) for i in P) for P in prefixes]
    levels = [{(): 0}]
    for P in prefixes:
        for d in range(1, len(P) + 1):
            if len(levels) <= d:
                levels.append({})
            levels[d].setdefault(P[:d], len(levels[d]))
    zero = np.float32(0)
    states = [np.maximum((lm.bh + lm.Wx[:, lm.bos]).astype(np.float32), zero)[None, :]]
    for d in range(1, len(levels)):
        keys = sorted(levels[d], key=levels[d].get)
        pre = (lm.bh[None, :] + lm.Wx[:, [P[-1] for P in keys]].T).astype(np.float32)
        par = states[d - 1][[levels[d - 1][P[:-1]] for P in keys]]
        states.append(np.maximum(matvec32(lm.Wh, pre, par), zero))
    out = np.stack([states[len(P)][levels[len(P)][P]] for P in prefixes]) if prefixes else np.zeros((0, lm.H), np.float32)
    z = matvec32(lm.Wo, lm.bo, out).astype(np.float64)
    return out, log10_softmax(z)


def symbol_rows(rows_v, sym_words):
    """[n, V] rows by LM id -> [n, A] rows by CTC symbol, column 0 (the blank) 0"""
    out = np.array(rows_v[:, np.asarray(sym_words)], copy=True)
    out[:, 0] = 0.0
    return out


def rows64(lm, sym_words):
    """lm_row for beam_model.decode: prefix of CTC symbols -> A float64 log10 values; the state of
    every prefix is cached, as clm_decoder2 caches it"""
    sw = np.asarray(sym_words)
    states, cache = {(): step64(lm, None, lm.bos)}, {}

    def state(P):
        if P not in states:
            states[P] = step64(lm, state(P[:-1]), sw[P[-1]])
        return states[P]

    def row(P):
        P = tuple(int(s) for s in P)
        if P not in cache:
            # no deep recursion on a long prefix whose ancestors were never asked for
            for d in range(len(P)):
                state(P[:d])
            cache[P] = symbol_rows(row64(lm, state(P))[None, :], sw)[0]
        return cache[P]
    return row


def spectral_norm(W):
    return float(np.linalg.norm(W.astype(np.float64), 2))


def random_lm(seed, V, H, scale=1.5, rho=0.9, chars=None):
    """an RNNCharLM with seeded weights: tokens <null> <s> </s> then ``chars`` (default c0, c1, ..);
    Wx N(0, scale^2 * 2), Wo N(0, scale^2 * 2 / H) so that the rows span several decades, and Wh drawn
    N(0, 1) and scaled to the spectral norm ``rho`` < 1"""
    import nn_lm
    rs = np.random.RandomState(seed)
    toks = ["<null>", "<s>", "</s>"] + (list(chars) if chars is not None else ["c%d" % i for i in range(V - 3)])
    assert len(toks) == V
    Wx = (rs.randn(H, V) * scale * np.sqrt(2.0)).astype(np.float32)
    Wh = rs.randn(H, H)
    Wh = (Wh * (rho / np.linalg.norm(Wh, 2))).astype(np.float32)
    bh = (0.1 * rs.randn(H)).astype(np.float32)
    Wo = (rs.randn(V, H) * scale * np.sqrt(2.0 / H)).astype(np.float32)
    bo = (0.1 * rs.randn(V)).astype(np.float32)
    return nn_lm.RNNCharLM(toks, Wx, Wh, bh, Wo, bo)
