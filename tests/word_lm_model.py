"""Plain-Python restatement of the word-LM second pass (csrc/word_lm_score.hip): the yardstick of
tests/test_gpu_word_lm_score.py and tests/test_gpu_word_rescore.py.  It works from label rows, the ``PrefixTree`` node
objects (not the flattened arrays) and ``LM.bg_prob`` / ``NgramLM.prob`` (not ``walk_packed``).

    tokens     maximal runs of symbols other than the space; no empty word (str.split())
    final_word a last token that no space follows is a word, unless ``final_word`` is False
    word id    walk the tree's nodes over the token: every step there and ``isWord`` at the end gives ``node.id``;
               anything else is OOV and gets ``lm.unk`` (None: status 3)
    term k     bigram LM: ``bg_prob(previous word, w)``, the previous word of word 0 is ``<s>``; a listed 0.0 is no value
               n-gram LM: ``prob(<s> + the words before, w)``; a listed 0.0 is a value
    eos        one more term P(</s> | history), no word
    sum        float64, terms added in word order; natural log
    status     2 for a symbol outside 1..A-1 (sum -inf, counts 0, no terms), 3 for an OOV word without <UNK> (sum -inf)

``mutate`` exists for the mutation checks of tests/test_word_lm_model_cpu.py only."""
import numpy as np

NEG = float("-inf")
MUTATIONS = ("drop_final", "no_start", "skip_oov", "zero_is_value", "count_eos")


def tokens_of(row, space):
    """[(symbols, a space follows)]"""
    out, cur = [], []
    for c in row:
        if c == space:
            if cur:
                out.append((cur, True))
            cur = []
        else:
            cur.append(c)
    if cur:
        out.append((cur, False))
    return out


def walk(tree, tok):
    """(node or None, steps taken): the walk stops at the first symbol without a child"""
    node = tree.root
    for i, c in enumerate(tok):
        if node.children is None or c not in node.children:
            return None, i
        node = node.children[c]
    return node, len(tok)


def _term(lm, ngram, hist, w, mutate):
    if ngram:
        return np.float32(lm.prob(hist, w))
    if not hist:                                                # the mutation without <s>
        return np.float32(lm.ug[w])
    if mutate == "zero_is_value" and (hist[-1], w) in lm.bg:
        return np.float32(lm.bg[(hist[-1], w)])
    return np.float32(lm.bg_prob(hist[-1], w))


def score_row(row, tree, lm, A, eos=False, final_word=True, mutate=None):
    """dict(sum float64, words, oov, status, terms [float32], ids [int])"""
    from decoder import ngram_lm
    ngram = isinstance(lm, ngram_lm.NgramLM)
    row = [int(c) for c in row]
    if any(not 1 <= c < A for c in row):
        return dict(sum=NEG, words=0, oov=0, status=2, terms=[], ids=[])
    ids, oov = [], 0
    for tok, spaced in tokens_of(row, int(tree.space)):
        if not spaced and (not final_word or mutate == "drop_final"):
            continue
        node, _ = walk(tree, tok)
        if node is not None and node.isWord:
            ids.append(int(node.id))
        elif mutate == "skip_oov":
            continue
        else:
            oov += 1
            ids.append(None if lm.unk is None else int(lm.unk))
    words = len(ids)
    if any(w is None for w in ids):
        return dict(sum=NEG, words=words, oov=oov, status=3, terms=[], ids=[])
    if eos:
        ids = ids + [int(lm.end)]
        words += 1 if mutate == "count_eos" else 0
    hist = [] if mutate == "no_start" else [int(lm.start)]
    terms, total = [], 0.0
    for w in ids:
        t = _term(lm, ngram, hist, w, mutate)
        terms.append(t)
        total = total + float(t)
        hist.append(w)
    return dict(sum=total, words=words, oov=oov, status=0, terms=terms, ids=ids)


def score_rows(rows, tree, lm, A, **kw):
    got = [score_row(r, tree, lm, A, **kw) for r in rows]
    return (np.array([g["sum"] for g in got], dtype=np.float64),
            np.array([[g["words"], g["oov"]] for g in got], dtype=np.int32).reshape(len(got), 2),
            np.array([g["status"] for g in got], dtype=np.int32), [g["terms"] for g in got], [g["ids"] for g in got])


def combine(total, lm_char, U, alpha, beta, word_sum, words, word_status, word_alpha, word_beta):
    """the second-pass objective, left to right in float64; a hypothesis the word LM cannot score is -inf outright"""
    if word_status != 0:
        return NEG
    first = (float(total) + float(alpha) * float(lm_char)) + float(beta) * float(U)
    return first + (float(word_alpha) * float(word_sum) + float(word_beta) * float(words))


def rank(total, status, lm, U, K_b, alpha, beta, wsum, wcount, wstatus, word_alpha, word_beta, first=None):
    """tests/rescore_model.rank with the word term: total, status, U, wsum, wstatus [B, K]; wcount [B, K, 2]; lm [B, K]
    or None -> (order int32 [B, K], rescored float64 [B, K])"""
    from tests import rescore_model
    total = np.asarray(total, dtype=np.float64)
    B, K = total.shape
    rescored = np.full((B, K), NEG, dtype=np.float64)
    order = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        kb = rescore_model.real_count(K_b[b], None if first is None else first[b])
        for k in range(kb):
            if status[b][k] == 0:
                rescored[b, k] = combine(total[b, k], 0.0 if lm is None else lm[b][k], U[b][k], alpha, beta, wsum[b][k],
                                         wcount[b][k][0], wstatus[b][k], word_alpha, word_beta)
        order[b] = sorted(range(kb), key=lambda k: (-rescored[b, k], k)) + list(range(kb, K))
    return order, rescored


# ---- the shared inputs -------------------------------------------------------------------------------------------------

LONG_WORD = "q" * 199          # in the test lexicon, so that a 200-symbol token can leave the tree at its last symbol
ONE_LETTER = "a t e o n u c f h p z k y w s d r j g q".split()


def spell(chars, text):
    """label row of a text: words of single-character tokens separated by single spaces; [name] is one symbol"""
    row = []
    for i, word in enumerate(text.split(" ")):
        if i:
            row.append(int(chars["[space]"]))
        if word.startswith("["):
            row.append(int(chars[word]))
        else:
            row.extend(int(chars[ch]) for ch in word)
    return row


def edge_rows(chars):
    """[(name, row)]: the rows that the issue of §4.14 lists, in the order of its list (the device-only case of two
    sequences sharing one ids range is built by the GPU test)"""
    sp = int(chars["[space]"])
    rs = np.random.RandomState(8191)
    lexicon_words = "eat a ntttn to tnt oot aoe noo eaa an".split()
    long_row = []
    while len(long_row) < 8191:
        word = lexicon_words[rs.randint(len(lexicon_words))] if rs.rand() < 0.7 else \
            "".join("aetonzq"[i] for i in rs.randint(0, 7, size=rs.randint(1, 7)))
        long_row.extend(spell(chars, word) + [sp])
    return [
        ("empty", []),
        ("spaces only", [sp, sp, sp]),
        ("leading, trailing and double spaces", [sp] + spell(chars, "a") + [sp, sp] + spell(chars, "eat to") + [sp]),
        ("a single special", spell(chars, "[laughter]")),
        ("a token across symbols 63 / 64", spell(chars, " ".join(["a"] * 30 + ["n", "ntttn", "eat"]))),
        ("200 symbols, off the tree at the third", spell(chars, "a na" + "z" * 198 + " eat")),
        ("200 symbols, off the tree at the last", spell(chars, "a " + LONG_WORD + "z eat")),
        ("70 one-letter words", spell(chars, " ".join(ONE_LETTER[i % len(ONE_LETTER)] for i in range(70)))),
        ("aoe, then an OOV", spell(chars, "eat aoe zzq to")),
        ("an OOV, then oot", spell(chars, "zzq oot a")),
        ("8191 symbols", long_row[:8191]),
    ]


def random_rows(chars, words, seed, n=24):
    """rows of lexicon words and made-up tokens: at least 20 % OOV and 50 % lexicon tokens (checked on the CPU)"""
    rs = np.random.RandomState(seed)
    letters = "aeton"
    rows = []
    for _ in range(n):
        toks = []
        for _ in range(rs.randint(0, 9)):
            if rs.rand() < 0.65:
                toks.append(words[rs.randint(len(words))])
            else:
                toks.append("".join(letters[i] for i in rs.randint(0, 5, size=rs.randint(4, 8))) + "zq")
        row = spell(chars, " ".join(toks)) if toks else []
        if rs.rand() < 0.3:
            row = [int(chars["[space]"])] + row
        if rs.rand() < 0.3:
            row = row + [int(chars["[space]"])]
        rows.append(row)
    return rows
