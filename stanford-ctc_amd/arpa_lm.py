"""ARPA n-gram language model for the prefix beam search decoder.

The reference's ``BeamLMDecoder`` scores characters with kenlm
(``ctc_fast/new_decoder/decoder.pyx:103-133``); kenlm is not a dependency here.  This
module reads the ARPA text format itself and scores with the standard back-off rule in
kenlm's order of float32 additions:

    log10 P(w | h) = p(longest h' w in the model) + bo(h'' for each longer context h''
                     of h that is in the model, shortest first)

``\\data\\`` / ``\\N-grams:`` sections, the back-off column optional (absent = 0).  Words
missing from the vocabulary score as ``<unk>``; a file without ``<unk>`` gets kenlm's
default unigram of -100.

For the GPU the model is packed into an open-addressing table of exact 64-bit keys:
word ids are 1..255 (0 = none), an n-gram w_1..w_n (oldest first) is
``w_1 << 8(n-1) | ... | w_n``, so order <= 8.  Each slot holds (key, log10 prob, log10
back-off); empty slots have key 0; the slot of a key is ``mix64(key) & (capacity-1)``,
then linear probing (``csrc/ctc_beam.hip`` walks the same table).
"""
import numpy as np

MAX_ORDER = 8
MAX_WORDS = 255
UNK_DEFAULT = -100.0      # kenlm's unigram probability of <unk> when the file has none

_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def mix64(keys):
    """splitmix64 finaliser over a uint64 array (wrap-around arithmetic, like the device)"""
    z = np.array(keys, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= _M1
        z ^= z >> np.uint64(27)
        z *= _M2
        z ^= z >> np.uint64(31)
    return z


def pack_ngram(ids):
    """exact 64-bit key of an n-gram given as word ids, oldest first"""
    k = 0
    for w in ids:
        k = (k << 8) | int(w)
    return k


class ArpaLM(object):
    """An ARPA back-off model: ``order``, ``words`` (id - 1 -> token), ``ngrams``
    ({tuple of ids: (float32 log10 prob, float32 log10 back-off)})."""

    def __init__(self, path=None, text=None):
        if text is None:
            with open(path) as f:
                text = f.read()
        self._parse(text)

    # ---- reading -----------------------------------------------------------------

    def _parse(self, text):
        counts = {}
        section = None
        rows = {}
        for raw in text.splitlines():
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                section = "data"
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:-len("-grams:")])
                rows[section] = []
                continue
            if section == "data":
                if line.startswith("ngram "):
                    n, c = line[len("ngram "):].split("=")
                    counts[int(n)] = int(c)
                continue
            if section is None:
                continue
            rows[section].append(line.split())
        if not rows or not counts:
            raise ValueError("not an ARPA file: no \\data\\ or no n-gram sections")
        self.order = max(rows)
        if self.order > MAX_ORDER:
            raise ValueError("ARPA order %d > %d" % (self.order, MAX_ORDER))
        for n in range(1, self.order + 1):
            if n not in rows:
                raise ValueError("ARPA file has no \\%d-grams: section" % n)
            if counts.get(n, len(rows[n])) != len(rows[n]):
                raise ValueError("ARPA \\data\\ says ngram %d=%d, the section has %d lines"
                                 % (n, counts[n], len(rows[n])))
        self.words = [r[1] for r in rows[1]]
        if "<unk>" not in self.words:
            self.words.append("<unk>")
        if len(self.words) > MAX_WORDS:
            raise ValueError("ARPA vocabulary of %d words > %d" % (len(self.words), MAX_WORDS))
        if "<s>" not in self.words:
            raise ValueError("ARPA vocabulary has no <s>")
        self.vocab = {w: i + 1 for i, w in enumerate(self.words)}
        self.unk = self.vocab["<unk>"]
        self.bos = self.vocab["<s>"]
        self.ngrams = {}
        for n in range(1, self.order + 1):
            for r in rows[n]:
                if len(r) not in (n + 1, n + 2):
                    raise ValueError("malformed %d-gram line: %s" % (n, " ".join(r)))
                ids = tuple(self.vocab[w] if w in self.vocab else self._unknown(w) for w in r[1:n + 1])
                bo = float(r[n + 1]) if len(r) == n + 2 else 0.0
                self.ngrams[ids] = (np.float32(float(r[0])), np.float32(bo))
        if (self.unk,) not in self.ngrams:
            self.ngrams[(self.unk,)] = (np.float32(UNK_DEFAULT), np.float32(0.0))

    def _unknown(self, w):
        raise ValueError("ARPA n-gram uses %r, which is not a unigram" % w)

    # ---- scoring ------------------------------------------------------------------

    def word_id(self, token):
        return self.vocab.get(token, self.unk)

    def score_ids(self, context, w):
        """float32 log10 P(w | context), context = word ids oldest first (``<s>`` included)"""
        ctx = tuple(context)[-(self.order - 1):] if self.order > 1 else ()
        p, n = self.ngrams[(w,)][0], 1
        for m in range(1, len(ctx) + 1):
            g = self.ngrams.get(ctx[len(ctx) - m:] + (w,))
            if g is None:
                break
            p, n = g[0], m + 1
        prob = np.float32(p)
        for m in range(n, len(ctx) + 1):
            g = self.ngrams.get(ctx[len(ctx) - m:])
            if g is None:
                break
            prob = np.float32(prob + g[1])
        return prob

    def full_scores(self, sentence, bos=True, eos=True):
        """kenlm.Model.full_scores: (log10 prob, n-gram length, oov) per word, then </s>"""
        toks = sentence.split()
        ctx = [self.bos] if bos else []
        if eos:
            toks = toks + ["</s>"]
        for t in toks:
            w = self.word_id(t)
            p = self.score_ids(ctx, w)
            yield float(p), 0, t not in self.vocab
            ctx.append(w)

    # ---- packing --------------------------------------------------------------------

    def pack(self):
        """(keys uint64[cap], prob float32[cap], backoff float32[cap]); cap a power of two
        with load factor <= 1/2"""
        n = len(self.ngrams)
        cap = 16
        while cap < 2 * n:
            cap *= 2
        items = list(self.ngrams.items())
        keys = np.array([pack_ngram(g) for g, _ in items], dtype=np.uint64)
        pv = np.array([v[0] for _, v in items], dtype=np.float32)
        bv = np.array([v[1] for _, v in items], dtype=np.float32)
        tk = np.zeros(cap, dtype=np.uint64)
        tp = np.zeros(cap, dtype=np.float32)
        tb = np.zeros(cap, dtype=np.float32)
        pos = (mix64(keys) & np.uint64(cap - 1)).astype(np.int64)
        todo = np.arange(n)
        while todo.size:
            free = tk[pos[todo]] == 0
            cand = todo[free]
            # one key per free slot per round: the first of each group
            _, first = np.unique(pos[cand], return_index=True)
            put = cand[first]
            tk[pos[put]] = keys[put]
            tp[pos[put]] = pv[put]
            tb[pos[put]] = bv[put]
            placed = np.zeros(n, dtype=bool)
            placed[put] = True
            todo = todo[~placed[todo]]
            pos[todo] = (pos[todo] + 1) & (cap - 1)
        return tk, tp, tb

    def symbol_words(self, int_char_map, A):
        """int32[A]: LM word id of each CTC symbol's token (0 for the blank and for ids
        without a token); tokens the LM does not know map to <unk>"""
        out = np.zeros(A, dtype=np.int32)
        for s in range(1, A):
            tok = int_char_map.get(s)
            out[s] = self.word_id(tok) if tok is not None else self.unk
        return out


def lookup_packed(table, key):
    """(prob, backoff) of ``key`` in a packed table, or None (host twin of the device walk)"""
    tk, tp, tb = table
    cap = tk.shape[0]
    s = int(mix64(np.array([key], dtype=np.uint64))[0]) & (cap - 1)
    while True:
        k = int(tk[s])
        if k == 0:
            return None
        if k == key:
            return tp[s], tb[s]
        s = (s + 1) & (cap - 1)
