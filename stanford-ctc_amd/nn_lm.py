"""Fixed-window feed-forward character LM for the prefix beam search decoder:
the neural LM of the reference's lexicon-free search (``ctc_fast/decoder/clm_decoder2.pyx``).

The reference's model classes are not part of its tree, so the model is defined here.  From
``clm_decoder2.pyx:43-71`` comes what that file does define, the context window and its padding:

    vocabulary  V tokens: ``<null>``, ``<s>``, ``</s>`` and the character tokens of chars.txt
    context     K slots (the reference's LM_ORDER - 1).  The last min(|P|, K) symbols of the prefix
                fill the newest slots; if |P| < K the slot before them holds ``<s>`` and every
                older slot ``<null>`` (clm_decoder2.pyx:52-54)
    input       the K one-hot vectors, oldest first: column ``slot * V + id`` of W0
    layers      h0 = relu(W0 x + b0), h_l = relu(W_l h_{l-1} + b_l), z = W_L h + b_L
    row         log10 softmax(z): log10, so that ``alpha`` means what it means for an ARPA LM

ReLU is this project's choice (the reference's nonlinearity lives in a repository that is not
there).  ``clm_decoder2`` multiplies natural logs: its alpha is this alpha divided by ln 10.

The model file is an ``.npz`` with ``tokens`` (V strings), ``context`` (K) and ``W0..WL`` /
``b0..bL`` (float32, W_l row-major [outputs][inputs]).  tools/train_char_nnlm.py writes one.

:class:`RNNCharLM` is the same search's ``rnn`` model type; its file says
``kind = "rnn"``, and :func:`load` returns the class a file asks for.
"""
import numpy as np

MAX_VOCAB = 256
MAX_CONTEXT = 32
MAX_HIDDEN_LAYERS = 4
MAX_WIDTH = 2048
SPECIALS = ("<null>", "<s>", "</s>")


class NNCharLM(object):
    """tokens: V strings; context: K; weights / biases: lists W0..WL / b0..bL."""

    def __init__(self, tokens, context, weights, biases):
        self.tokens = [str(t) for t in tokens]
        self.V = len(self.tokens)
        self.context = int(context)
        self.weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        if not 3 <= self.V <= MAX_VOCAB:
            raise ValueError("NNCharLM: vocabulary of %d tokens outside 3..%d" % (self.V, MAX_VOCAB))
        if len(set(self.tokens)) != self.V:
            raise ValueError("NNCharLM: a token is listed twice")
        for t in SPECIALS:
            if t not in self.tokens:
                raise ValueError("NNCharLM: the vocabulary has no %s" % t)
        if not 1 <= self.context <= MAX_CONTEXT:
            raise ValueError("NNCharLM: context %d outside 1..%d" % (self.context, MAX_CONTEXT))
        n = len(self.weights)
        if len(self.biases) != n or not 2 <= n <= MAX_HIDDEN_LAYERS + 1:
            raise ValueError("NNCharLM: %d weight matrices and %d biases; 1..%d hidden layers and the "
                             "output layer are expected" % (n, len(self.biases), MAX_HIDDEN_LAYERS))
        width = self.context * self.V
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.ndim != 2 or w.shape[1] != width or b.shape[0] != w.shape[0]:
                raise ValueError("NNCharLM: W%d is %s and b%d %s, %d inputs are expected"
                                 % (l, w.shape, l, b.shape, width))
            width = w.shape[0]
            if l < n - 1 and not 1 <= width <= MAX_WIDTH:
                raise ValueError("NNCharLM: hidden width %d outside 1..%d" % (width, MAX_WIDTH))
        if width != self.V:
            raise ValueError("NNCharLM: the output layer has %d units, the vocabulary %d tokens" % (width, self.V))
        self.vocab = {t: i for i, t in enumerate(self.tokens)}
        self.null, self.bos, self.eos = (self.vocab[t] for t in SPECIALS)

    # ---- the model file ---------------------------------------------------------------

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            n = 0
            while "W%d" % n in z.files:
                n += 1
            return cls([str(t) for t in z["tokens"]], int(z["context"]), [z["W%d" % l] for l in range(n)],
                       [z["b%d" % l] for l in range(n)])

    def save(self, path):
        arrs = {"tokens": np.array(self.tokens), "context": np.int32(self.context)}
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            arrs["W%d" % l] = w
            arrs["b%d" % l] = b
        with open(path, "wb") as f:          # a file object: savez appends no suffix of its own
            np.savez(f, **arrs)

    # ---- contexts ---------------------------------------------------------------------

    def context_ids(self, prefix_lm_ids):
        """the K LM ids of the window of a prefix given as LM ids, oldest slot first"""
        K = self.context
        tail = [int(i) for i in prefix_lm_ids][-K:]
        if len(tail) < K:
            tail = [self.null] * (K - len(tail) - 1) + [self.bos] + tail
        return np.asarray(tail, dtype=np.int32)

    def symbol_words(self, int_char_map, A):
        """int32[A]: LM id of each CTC symbol's token (0 for the blank, which is never asked).
        A symbol without a token, or whose token the LM does not know, is a ValueError: the
        search could never extend it (``clm_decoder2`` silently does just that)."""
        out = np.zeros(A, dtype=np.int32)
        for s in range(1, A):
            tok = int_char_map.get(s)
            if tok is None or tok not in self.vocab:
                raise ValueError("NNCharLM: symbol %d (%r) has no token in the LM's vocabulary" % (s, tok))
            out[s] = self.vocab[tok]
        return out

    # ---- what the device gets ---------------------------------------------------------

    def padded(self):
        """(widths, weights, biases) with every hidden width zero-padded to a multiple of 32.  The
        padding is exact: a padded unit is relu(0) = 0 and its outgoing weights are 0."""
        ws, bs = [], []
        widths = [self.context * self.V]
        n = len(self.weights)
        for l, (w, b) in enumerate(zip(self.weights, self.biases)):
            rows = w.shape[0] if l == n - 1 else (w.shape[0] + 31) // 32 * 32
            wp = np.zeros((rows, widths[-1]), dtype=np.float32)
            wp[:w.shape[0], :w.shape[1]] = w
            bp = np.zeros(rows, dtype=np.float32)
            bp[:b.shape[0]] = b
            ws.append(wp)
            bs.append(bp)
            widths.append(rows)
        return np.asarray(widths, dtype=np.int32), ws, bs


class RNNCharLM(object):
    """The recurrent character LM of DESIGN.md §4.10, the ``rnn`` model type of ``clm_decoder2.pyx``
    (its lines 43-80): the hidden state is a function of the prefix, cached per prefix by the search.

        h(())  = relu(bh + Wx[:, <s>] + Wh 0)                 the empty prefix feeds <s> into no state
        h(P)   = relu(bh + Wx[:, id(P[-1])] + Wh h(P[:-1]))   a prefix feeds its last symbol only
        row(P) = log10 softmax(Wo h(P) + bo)

    ReLU and log10 as for :class:`NNCharLM`.  The model file is an ``.npz`` with ``kind = "rnn"``,
    ``tokens`` (V strings, the rule of NNCharLM; ``<null>`` is never fed) and ``Wx [H][V]``,
    ``Wh [H][H]``, ``bh [H]``, ``Wo [V][H]``, ``bo [V]`` (float32).  tools/train_char_nnlm.py --rnn
    writes one."""

    def __init__(self, tokens, Wx, Wh, bh, Wo, bo):
        self.tokens = [str(t) for t in tokens]
        self.V = len(self.tokens)
        self.Wx, self.Wh, self.Wo = (np.ascontiguousarray(w, dtype=np.float32) for w in (Wx, Wh, Wo))
        self.bh, self.bo = (np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in (bh, bo))
        if not 3 <= self.V <= MAX_VOCAB:
            raise ValueError("RNNCharLM: vocabulary of %d tokens outside 3..%d" % (self.V, MAX_VOCAB))
        if len(set(self.tokens)) != self.V:
            raise ValueError("RNNCharLM: a token is listed twice")
        for t in SPECIALS:
            if t not in self.tokens:
                raise ValueError("RNNCharLM: the vocabulary has no %s" % t)
        if self.Wx.ndim != 2 or not 1 <= self.Wx.shape[0] <= MAX_WIDTH:
            raise ValueError("RNNCharLM: Wx is %s; [H][V] with H in 1..%d is expected" % (self.Wx.shape, MAX_WIDTH))
        self.H = H = self.Wx.shape[0]
        for name, a, shape in (("Wx", self.Wx, (H, self.V)), ("Wh", self.Wh, (H, H)), ("bh", self.bh, (H,)),
                               ("Wo", self.Wo, (self.V, H)), ("bo", self.bo, (self.V,))):
            if a.shape != shape:
                raise ValueError("RNNCharLM: %s is %s, %s is expected" % (name, a.shape, shape))
        self.vocab = {t: i for i, t in enumerate(self.tokens)}
        self.null, self.bos, self.eos = (self.vocab[t] for t in SPECIALS)

    symbol_words = NNCharLM.symbol_words

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "kind" not in z.files or str(z["kind"]) != "rnn":
                raise ValueError("RNNCharLM: %s is not a recurrent model file (kind = \"rnn\")" % path)
            return cls([str(t) for t in z["tokens"]], z["Wx"], z["Wh"], z["bh"], z["Wo"], z["bo"])

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, kind=np.array("rnn"), tokens=np.array(self.tokens), Wx=self.Wx, Wh=self.Wh, bh=self.bh,
                     Wo=self.Wo, bo=self.bo)

    def padded(self):
        """(Hp, Wx, Wh, bh, Wo) with H zero-padded to a multiple of 32.  The padding is exact: a padded
        unit is relu(0) = 0 and its outgoing weights are 0."""
        H, Hp = self.H, (self.H + 31) // 32 * 32
        Wx = np.zeros((Hp, self.V), dtype=np.float32)
        Wh = np.zeros((Hp, Hp), dtype=np.float32)
        bh = np.zeros(Hp, dtype=np.float32)
        Wo = np.zeros((self.V, Hp), dtype=np.float32)
        Wx[:H], Wh[:H, :H], bh[:H], Wo[:, :H] = self.Wx, self.Wh, self.bh, self.Wo
        return Hp, Wx, Wh, bh, Wo


def load(path):
    """the model of an ``.npz`` file: an :class:`RNNCharLM` when its ``kind`` says "rnn", else (no
    ``kind``) the feed-forward :class:`NNCharLM`"""
    with np.load(path, allow_pickle=False) as z:
        kind = str(z["kind"]) if "kind" in z.files else None
    if kind is None:
        return NNCharLM.load(path)
    if kind == "rnn":
        return RNNCharLM.load(path)
    raise ValueError("nn_lm.load: %s has the unknown kind %r" % (path, kind))
