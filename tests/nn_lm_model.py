"""Float64 restatement of the feed-forward character LM of DESIGN.md §4.7 (nn_lm.NNCharLM), the
yardstick of the neural-LM decoder tests: the context rule, the forward pass written as matrix
products over an explicit one-hot input, and the log10 softmax.  ``rows64(lm, sym_words)`` is an
``lm_row(prefix)`` provider for the unmodified tests/beam_model.decode and beam_trace.model_trace.

``forward32`` is the float32 evaluation that accumulates every sum in ascending k: the distance
d32 = max |forward32 - forward64| over a set of contexts is what float32 arithmetic of this model
costs, and the device may deviate from float64 by at most twice that."""
import numpy as np

LOG10E = 0.43429448190325182765


def reference_context(tokens_of_prefix, order):
    """A literal re-reading of clm_decoder2.pyx:52-54 (the non-rnn branch), on token strings:
        s = int_to_char(prefix[-order+1:], char_map)
        if len(s) < order - 1:
            s = ['<null>'] * (order - len(s) - 2) + ['<s>'] + s
    order = LM_ORDER = K + 1.  ``prefix[-0:]`` is the whole prefix in Python, which for order 1
    would leave a window of unbounded length: K = 0 is not a model here."""
    prefix = list(tokens_of_prefix)
    s = prefix[-order + 1:]
    if len(s) < order - 1:
        s = ['<null>'] * (order - len(s) - 2) + ['<s>'] + s
    return s


def one_hot_input(lm, ctx_ids, dtype=np.float64):
    """x of §1: the K one-hot vectors concatenated oldest first"""
    x = np.zeros(lm.context * lm.V, dtype=dtype)
    for slot, i in enumerate(ctx_ids):
        x[slot * lm.V + int(i)] = 1.0
    return x


def forward64(lm, ctx_ids, weights=None, biases=None):
    """float64 log10 softmax row of one window of LM ids, with the input matrix formed"""
    ws = lm.weights if weights is None else weights
    bs = lm.biases if biases is None else biases
    h = one_hot_input(lm, ctx_ids)
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = w.astype(np.float64) @ h + b.astype(np.float64)
        if l < len(ws) - 1:
            h = np.maximum(h, 0.0)
    h = h[:lm.V]
    m = h.max()
    return (h - (m + np.log(np.exp(h - m).sum()))) * LOG10E


def forward32(lm, contexts):
    """float32 rows [n, V] of int windows [n, K]: every sum accumulated in float32 in ascending k
    (one rounded multiply and one rounded add per term), the log-softmax in float64"""
    ctx = np.asarray(contexts).reshape(-1, lm.context)
    n = ctx.shape[0]
    w0, b0 = lm.weights[0], lm.biases[0]
    h = np.tile(b0.astype(np.float32), (n, 1))
    for slot in range(lm.context):
        h = (h + w0[:, slot * lm.V + ctx[:, slot]].T).astype(np.float32)
    h = np.maximum(h, np.float32(0))
    for l in range(1, len(lm.weights)):
        w, b = lm.weights[l], lm.biases[l]
        acc = np.tile(b.astype(np.float32), (n, 1))
        for k in range(w.shape[1]):
            acc = (acc + (h[:, k:k + 1] * w[:, k][None, :]).astype(np.float32)).astype(np.float32)
        h = np.maximum(acc, np.float32(0)) if l < len(lm.weights) - 1 else acc
    z = h.astype(np.float64)
    m = z.max(axis=1, keepdims=True)
    return ((z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))) * LOG10E)


def rows64_of_contexts(lm, contexts):
    return np.stack([forward64(lm, c) for c in np.asarray(contexts).reshape(-1, lm.context)])


def symbol_rows(rows_v, sym_words):
    """[n, V] rows by LM id -> [n, A] rows by CTC symbol, column 0 (the blank) 0"""
    out = np.array(rows_v[:, np.asarray(sym_words)], copy=True)
    out[:, 0] = 0.0
    return out


def rows64(lm, sym_words):
    """lm_row for beam_model.decode: prefix of CTC symbols -> A float64 log10 values"""
    sw = np.asarray(sym_words)
    cache = {}

    def row(P):
        ctx = tuple(int(i) for i in lm.context_ids([sw[s] for s in P]))
        if ctx not in cache:
            cache[ctx] = symbol_rows(forward64(lm, ctx)[None, :], sw)[0]
        return cache[ctx]
    return row


def random_lm(seed, V, K, hidden, scale=1.0, chars=None):
    """an NNCharLM with seeded weights: tokens <null> <s> </s> then ``chars`` (default c0, c1, ..),
    N(0, scale^2 * 2 / fan_in) weights so that rows span several decades whatever the widths"""
    import nn_lm
    rs = np.random.RandomState(seed)
    toks = ["<null>", "<s>", "</s>"] + (list(chars) if chars is not None else ["c%d" % i for i in range(V - 3)])
    assert len(toks) == V
    widths = [K * V] + list(hidden) + [V]
    ws, bs = [], []
    for l in range(len(widths) - 1):
        fan = K if l == 0 else widths[l]
        ws.append((rs.randn(widths[l + 1], widths[l]) * scale * np.sqrt(2.0 / fan)).astype(np.float32))
        bs.append((0.1 * rs.randn(widths[l + 1])).astype(np.float32))
    return nn_lm.NNCharLM(toks, K, ws, bs)
