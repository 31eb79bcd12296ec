#!/usr/bin/env python3
"""Generate the prefix beam search fixtures under tests/golden/ from the REFERENCE'S OWN
decoder.

The unmodified ``ctc_fast/new_decoder/decoder.pyx`` of the reference checkout is
cythonized (language_level=2) in a scratch directory OUTSIDE the repository.  Two small
modules of this script's own make it run under Python 3:

* ``collections``: a shim whose ``defaultdict`` has ``iteritems`` (decoder.pyx:162 sorts
  ``Hnext.iteritems()``), assigned as ``decoder.collections``;
* ``kenlm``: kenlm itself is not available, so a stand-in ``LanguageModel`` whose
  ``full_scores`` is backed by this project's ARPA scorer (stanford-ctc_amd/arpa_lm.py).
  The LM terms of the fixtures are therefore pinned to the ARPA back-off formula (in
  kenlm's float32 order of additions), not to kenlm's binary.

Fixtures written:
  lm_char_2g.arpa, lm_char_5g.arpa  character LMs built here from a synthetic corpus
                                    (absolute discounting, Katz back-off; the 2-gram has no
                                    <unk>, the 5-gram has one and pruned 3..5-grams)
  chars.txt                         ``token id`` lines (decoder.pyx:44-59), symbol 4
                                    ``[laughter]`` is unknown to both LMs
  decode_ref.npz                    per case: inputs, the reference's hypothesis (symbol ids)
                                    and score, and the top-2 key margin of the final beam
                                    (from tests/beam_model.py: the reference returns only the
                                    top entry); hypotheses are compared only where the margin
                                    is >= 1e-6, scores always
  decode_ref_trace.npz              a second case list (TRACE_CASES) with alpha and beta that are
                                    not float32 numbers: per case the inputs and, for EVERY
                                    truncation lp[:, :t], t = 1..T, the reference's hypothesis
                                    (symbol ids, concatenated; ``len`` splits them) and score --
                                    the reference's top entry after every frame

The two case lists draw from generators of their own, so decode_ref.npz does not depend on the
second list.  The committed decode_ref.npz predates the float64 alpha * LM product of
tests/beam_model.py: a regenerated file has every array of the reference equal (lp, cfg, hyp, score)
and the model-derived ``margin`` of the six alpha = 1.5 cases moved by at most 6e-8, far from the
1e-6 they are compared with, so the committed file was left as it is.  --out DIR writes
everything elsewhere (to compare with the committed files).

Usage:  python tests/golden/make_golden_decode.py --reference <reference checkout> [--scratch DIR]
                                                  [--out DIR]
"""
import argparse
import collections as _collections
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "stanford-ctc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import arpa_lm  # noqa: E402
import beam_model  # noqa: E402

TOKENS = ["[space]", "a", "e", "[laughter]", "t", "o", "n", "i", "s", "h", "r", "d", "l", "u",
          "c", "m", "w", "f", "g", "y", "p", "b", "v", "k", "'", "j", "x", "q", "z", "-", ".",
          "[noise]", "[vocalized-noise]", "&"]          # symbols 1..34; A = 35 with the blank
UNKNOWN = {"[laughter]", "&"}


# ---- the reference, built in scratch ------------------------------------------------------

KENLM_STANDIN = '''"""kenlm stand-in: LanguageModel(path).full_scores(sentence) from the project's ARPA scorer"""
import arpa_lm


class LanguageModel(object):
    def __init__(self, path):
        self.lm = arpa_lm.ArpaLM(path)
        self._ctx = {}

    def full_scores(self, sentence, bos=True, eos=True):
        lm = self.lm
        toks = sentence.split()
        # decoder.pyx scores prefix + one symbol over and over: keep the scores of each prefix
        head = " ".join(toks[:-1])
        got = self._ctx.get(head)
        if got is None:
            got = list(lm.full_scores(head, bos=bos, eos=False)) if toks[:-1] else []
            self._ctx[head] = got
        ctx = ([lm.bos] if bos else []) + [lm.word_id(t) for t in toks[:-1]]
        w = lm.word_id(toks[-1])
        out = got + [(float(lm.score_ids(ctx, w)), 0, toks[-1] not in lm.vocab)]
        if eos:
            out.append((float(lm.score_ids(ctx + [w], lm.word_id("</s>"))), 0, False))
        return out
'''


class _DefaultDict(_collections.defaultdict):
    def iteritems(self):
        return iter(self.items())


class _CollectionsShim(object):
    defaultdict = _DefaultDict


def build_reference(ref, scratch):
    os.makedirs(scratch, exist_ok=True)
    pyx = os.path.join(ref, "ctc_fast/new_decoder/decoder.pyx")
    setup = os.path.join(scratch, "setup_decoder.py")
    with open(setup, "w") as f:
        f.write(
            "from setuptools import setup, Extension\n"
            "from Cython.Build import cythonize\n"
            "import numpy as np\n"
            "setup(ext_modules=cythonize([Extension('decoder', [%r],\n"
            "      include_dirs=[np.get_include()])], language_level=2, build_dir=%r))\n"
            % (pyx, os.path.join(scratch, "cy_dec")))
    with open(os.path.join(scratch, "kenlm.py"), "w") as f:
        f.write(KENLM_STANDIN)
    if not any(n.startswith("decoder.") and n.endswith(".so") for n in os.listdir(scratch)):
        subprocess.check_call([sys.executable, setup, "build_ext", "--build-lib", scratch,
                               "--build-temp", os.path.join(scratch, "tmp_dec")], cwd=scratch,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, scratch)
    import decoder  # noqa: the reference's Cython module
    decoder.collections = _CollectionsShim
    return decoder


# ---- synthetic character LMs ------------------------------------------------------------

def corpus(rs, n_sent=400):
    letters = [t for t in TOKENS if t not in UNKNOWN and t != "[space]"][:24]
    lex = ["".join(rs.choice(list("aetonishrdlucmwfgyp"), size=rs.randint(1, 7))) for _ in range(120)]
    sents = []
    for _ in range(n_sent):
        words = [lex[min(int(rs.zipf(1.3)) - 1, len(lex) - 1)] for _ in range(rs.randint(1, 8))]
        toks = []
        for i, w in enumerate(words):
            if i:
                toks.append("[space]")
            toks.extend(list(w))
        if rs.rand() < 0.1:
            toks.append(letters[rs.randint(len(letters))])
        sents.append(toks)
    return sents


def build_arpa(sents, order, min_count, with_unk, D=0.5):
    counts = [None] + [_collections.Counter() for _ in range(order)]
    for s in sents:
        seq = ["<s>"] + s + ["</s>"]
        for n in range(1, order + 1):
            for i in range(len(seq) - n + 1):
                g = tuple(seq[i:i + n])
                if n == 1 and g == ("<s>",):
                    continue
                if g[1:].count("<s>") or (g[-1] != "</s>" and "</s>" in g):
                    continue
                counts[n][g] += 1
    keep = [None, dict(counts[1])]
    for n in range(2, order + 1):
        keep.append({g: c for g, c in counts[n].items()
                     if c >= (min_count if n >= 3 else 1) and g[:-1] in keep[n - 1] | {("<s>",): 0}
                     and g[1:] in keep[n - 1]})
    total = sum(keep[1].values())
    extra = 1e-4 if with_unk else 0.0
    prob = {}
    for g, c in keep[1].items():
        prob[g] = np.log10((1 - extra) * c / total)
    if with_unk:
        prob[("<unk>",)] = np.log10(extra)
    prob[("<s>",)] = -99.0
    bo = {}

    def p_lower(h, w):           # full back-off probability (float64) of w after context h
        if h + (w,) in prob:
            return 10.0 ** prob[h + (w,)]
        if not h:
            return 10.0 ** prob.get((w,), -99.0)
        return 10.0 ** bo.get(h, 0.0) * p_lower(h[1:], w)

    for n in range(2, order + 1):
        ctx_tot = _collections.Counter()
        for g, c in counts[n].items():
            ctx_tot[g[:-1]] += c
        by_ctx = _collections.defaultdict(list)
        for g, c in keep[n].items():
            by_ctx[g[:-1]].append((g, c))
        for h, gs in by_ctx.items():
            tot = ctx_tot[h]
            s_hi = s_lo = 0.0
            for g, c in gs:
                p = (c - D) / tot
                prob[g] = np.log10(p)
                s_hi += p
                s_lo += p_lower(h[1:], g[-1])
            bo[h] = float(np.log10(max(1e-12, 1 - s_hi) / max(1e-12, 1 - s_lo)))
    lines = ["\\data\\"]
    grams = [None] + [[g for g in prob if len(g) == n] for n in range(1, order + 1)]
    for n in range(1, order + 1):
        lines.append("ngram %d=%d" % (n, len(grams[n])))
    for n in range(1, order + 1):
        lines += ["", "\\%d-grams:" % n]
        for g in sorted(grams[n]):
            row = "%.6f\t%s" % (prob[g], " ".join(g))
            if n < order and g in bo:            # no column where the n-gram is no context
                row += "\t%.6f" % bo[g]
            lines.append(row)
    lines += ["", "\\end\\", ""]
    return "\n".join(lines)


# ---- cases -----------------------------------------------------------------------------

def logsoftmax(x):
    m = x.max(axis=0, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))


def posteriors(rs, A, T, kind):
    if kind == "flat":
        return logsoftmax(0.4 * rs.randn(A, T))
    if kind == "blank":
        x = rs.randn(A, T)
        x[0] += 12.0
        return logsoftmax(x)
    x = 1.5 * rs.randn(A, T)
    t = 0
    while t < T:                                 # a random path: runs of symbols and blanks
        s = rs.randint(1, A) if rs.rand() < 0.6 else 0
        r = rs.randint(1, 4)
        x[s, t:t + r] += 6.0
        t += r
    lp = logsoftmax(x)
    if kind == "neginf":
        mask = rs.rand(A, T) < 0.15
        mask[np.argmax(lp, axis=0), np.arange(T)] = False
        lp[mask] = -np.inf
    if kind == "missing":                        # the LM-unknown symbol 4 is likely
        lp = logsoftmax(np.where(np.arange(A)[:, None] == 4, x + 5.0, x))
    return lp


CASES = [   # (A, T, beam, alpha, beta, lm, kind)
    (35, 1, 16, 0.5, 0.0, "2g", "peaked"),
    (35, 2, 16, 1.5, 1.5, "5g", "peaked"),
    (8, 5, 1, 0.0, 0.0, "2g", "peaked"),
    (8, 12, 16, 0.5, 0.0, "2g", "flat"),
    (8, 40, 150, 1.5, 1.5, "5g", "flat"),
    (8, 300, 1, 0.5, 1.5, "2g", "peaked"),
    (8, 300, 16, 1.5, 0.0, "5g", "peaked"),
    (8, 60, 16, 0.0, 0.0, "5g", "blank"),
    (8, 30, 16, 0.5, 0.0, "2g", "neginf"),
    (8, 40, 16, 1.5, 0.0, "2g", "missing"),
    (33, 20, 1, 0.0, 0.0, "2g", "flat"),
    (33, 60, 16, 0.5, 0.0, "2g", "peaked"),
    (33, 120, 16, 1.5, 1.5, "5g", "peaked"),
    (33, 200, 1, 1.5, 0.0, "5g", "peaked"),
    (33, 25, 150, 0.5, 0.0, "5g", "peaked"),
    (33, 30, 16, 0.0, 1.5, "2g", "neginf"),
    (33, 40, 16, 0.5, 1.5, "5g", "blank"),
    (33, 50, 16, 1.5, 0.0, "2g", "missing"),
    (33, 15, 150, 1.5, 0.0, "2g", "flat"),
    (33, 300, 16, 0.5, 0.0, "2g", "peaked"),
    (35, 10, 16, 0.5, 0.0, "5g", "flat"),
    (35, 30, 150, 0.0, 0.0, "2g", "peaked"),
    (35, 40, 150, 0.5, 1.5, "5g", "peaked"),
    (35, 20, 150, 1.5, 0.0, "5g", "flat"),
    (35, 100, 1, 0.5, 0.0, "5g", "peaked"),
    (35, 150, 16, 1.5, 1.5, "2g", "peaked"),
    (35, 300, 16, 0.0, 0.0, "5g", "peaked"),
    (35, 250, 1, 1.5, 1.5, "2g", "peaked"),
    (35, 50, 16, 0.5, 0.0, "2g", "blank"),
    (35, 30, 150, 1.5, 0.0, "2g", "blank"),
    (35, 40, 16, 1.5, 0.0, "5g", "neginf"),
    (35, 35, 150, 0.5, 1.5, "5g", "neginf"),
    (35, 60, 16, 0.5, 0.0, "5g", "missing"),
    (35, 30, 150, 1.5, 1.5, "2g", "missing"),
    (35, 80, 16, 0.0, 1.5, "2g", "flat"),
    (35, 200, 16, 0.5, 1.5, "5g", "peaked"),
    (35, 45, 40, 1.0, 0.0, "5g", "peaked"),
    (35, 45, 40, 1.0, 0.0, "2g", "flat"),
    (33, 70, 40, 0.5, 0.0, "5g", "missing"),
    (8, 100, 40, 0.5, 1.5, "2g", "neginf"),
]


TRACE_CASES = [   # (A, T, beam, alpha, beta, lm, kind): every truncation is decoded
    (35, 40, 40, 0.8, 0.37, "5g", "peaked"),
    (35, 40, 16, 1.3, 0.0, "2g", "peaked"),
    (8, 40, 40, 1.3, 0.0, "5g", "flat"),
    (8, 40, 16, 0.8, 0.37, "2g", "peaked"),
    (35, 36, 16, 1.3, 0.37, "5g", "missing"),
    (35, 30, 40, 0.8, 0.0, "2g", "missing"),
]


def split_ids(hyp, int_char, A):
    """the reference's string back to symbol ids (tokens are distinct, at most one per symbol;
    '[...]' tokens are multi-character, so match greedily against the map)"""
    ids = []
    pos = 0
    by_len = sorted(int_char.items(), key=lambda kv: -len(kv[1]))
    while pos < len(hyp):
        for s, tok in by_len:
            if hyp.startswith(tok, pos) and s < A:
                ids.append(s)
                pos += len(tok)
                break
        else:
            raise AssertionError("cannot split %r" % hyp)
    return ids


def trace_cases(dec, chars, out_dir, int_char):
    rs = np.random.RandomState(4202)
    out = {"n": np.int64(len(TRACE_CASES))}
    for i, (A, T, beam, alpha, beta, lmk, kind) in enumerate(TRACE_CASES):
        assert float(np.float32(alpha)) != alpha
        d = dec.BeamLMDecoder()
        d.load_chars(chars)
        d.load_lm(os.path.join(out_dir, "lm_char_%s.arpa" % lmk))
        lp = posteriors(rs, A, T, kind)
        t0 = time.time()
        ids, lens, scores = [], [], []
        for t in range(1, T + 1):
            hyp, score = d.decode(np.asfortranarray(lp[:, :t]), beam, alpha, beta)
            h = split_ids(hyp, int_char, A)
            ids += h
            lens.append(len(h))
            scores.append(score)
        print("trace case %d A=%2d T=%2d beam=%2d alpha=%.2f beta=%.2f %s %-7s final score %.6f %.1fs"
              % (i, A, T, beam, alpha, beta, lmk, kind, scores[-1], time.time() - t0))
        out["lp%d" % i] = lp
        out["cfg%d" % i] = np.array([A, T, beam, alpha, beta], dtype=np.float64)
        out["lm%d" % i] = np.array(lmk)
        out["kind%d" % i] = np.array(kind)
        out["hyp%d" % i] = np.array(ids, dtype=np.int32)
        out["len%d" % i] = np.array(lens, dtype=np.int32)
        out["score%d" % i] = np.array(scores, dtype=np.float64)
    np.savez_compressed(os.path.join(out_dir, "decode_ref_trace.npz"), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--scratch", default="/tmp/sctc_ref_decoder")
    ap.add_argument("--out", default=HERE, help="where the fixtures are written")
    a = ap.parse_args()
    assert not os.path.abspath(a.scratch).startswith(ROOT), "scratch must be outside the repo"
    OUT = os.path.abspath(a.out)
    os.makedirs(OUT, exist_ok=True)
    rs = np.random.RandomState(2024)
    sents = corpus(rs)
    lm_text = {"2g": build_arpa(sents, 2, 1, with_unk=False),
               "5g": build_arpa(sents, 5, 2, with_unk=True)}
    for k, txt in lm_text.items():
        with open(os.path.join(OUT, "lm_char_%s.arpa" % k), "w") as f:
            f.write(txt)
    chars = os.path.join(OUT, "chars.txt")
    with open(chars, "w") as f:
        for i, t in enumerate(TOKENS):
            f.write("%s %d\n" % (t, i + 1))
    dec = build_reference(a.reference, a.scratch)
    lms = {k: arpa_lm.ArpaLM(os.path.join(OUT, "lm_char_%s.arpa" % k)) for k in lm_text}
    int_char = {i + 1: t for i, t in enumerate(TOKENS)}
    out = {"n": np.int64(len(CASES))}
    with np.errstate(all="ignore"):
        for i, (A, T, beam, alpha, beta, lmk, kind) in enumerate(CASES):
            d = dec.BeamLMDecoder()
            d.load_chars(chars)
            d.load_lm(os.path.join(OUT, "lm_char_%s.arpa" % lmk))
            lp = np.asfortranarray(posteriors(rs, A, T, kind))
            t0 = time.time()
            hyp, score = d.decode(lp, beam, alpha, beta)
            dt = time.time() - t0
            ids = split_ids(hyp, int_char, A)
            sw = lms[lmk].symbol_words(int_char, A)
            top2 = beam_model.decode(lp, beam, alpha, beta, beam_model.arpa_rows(lms[lmk], sw), nbest=2)
            margin = top2[0][1] - top2[1][1] if len(top2) > 1 else np.inf
            agree = list(top2[0][0]) == ids
            print("case %2d A=%2d T=%3d beam=%3d alpha=%.1f beta=%.1f %s %-7s score %.6f margin %.3g "
                  "model %s %.1fs" % (i, A, T, beam, alpha, beta, lmk, kind, score, margin,
                                      "agrees" if agree else "DIFFERS", dt))
            assert score > -700, score
            out["lp%d" % i] = lp
            out["cfg%d" % i] = np.array([A, T, beam, alpha, beta], dtype=np.float64)
            out["lm%d" % i] = np.array(lmk)
            out["kind%d" % i] = np.array(kind)
            out["hyp%d" % i] = np.array(ids, dtype=np.int32)
            out["hyps%d" % i] = np.array(hyp)
            out["score%d" % i] = np.float64(score)
            out["margin%d" % i] = np.float64(margin)
        np.savez_compressed(os.path.join(OUT, "decode_ref.npz"), **out)
        trace_cases(dec, chars, OUT, int_char)


if __name__ == "__main__":
    main()
