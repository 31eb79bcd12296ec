"""Perplexity of a text under a character LM, on the GPU: the reference's
ctc_fast/clm/clm_pp.py for the three LMs of this project.  The text holds one sentence per line,
space-separated character tokens as in chars.txt (``[space]`` for the blank between words), the format
tools/train_char_nnlm.py trains from.  Every sentence is scored from ``<s>`` to ``</s>`` (``--no-eos``: without
the ``</s>`` term); tokens the LM does not know count as ``<unk>`` under an ARPA LM and are an error under a
neural one.  Prints ``perplexity``, ``bits per character`` and the number of terms.

    python tools/lm_perplexity.py --text text.txt --chars chars.txt --lm {lm.arpa | lm.npz} [--no-eos]

``--word-lm ARPA --words WORDLIST [--word-lm-order N]`` in place of ``--lm``: the word-level perplexity of the same
text under a word LM.  The words are the runs of tokens between ``[space]`` tokens; a word outside
WORDLIST counts as ``<UNK>``.  Prints ``perplexity`` (e ** (-sum of the natural-log terms / terms)), the number of terms
and the number of OOV words.

    python tools/lm_perplexity.py --text text.txt --chars chars.txt --word-lm words.arpa --words words.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import arpa_lm  # noqa: E402
import ctc_fast  # noqa: E402
import nn_lm  # noqa: E402


def word_perplexity(a):
    from decoder import decoder_utils
    chars = decoder_utils.load_chars(a.chars)
    lex = ctc_fast.DecodeLexicon(a.words, chars, a.word_lm, a.space, specials=a.specials, order=a.word_lm_order)
    with open(a.text) as f:
        lines = [line.split() for line in f if line.strip()]
    for toks in lines:
        for t in toks:
            if t not in chars:
                raise SystemExit("lm_perplexity: %r is no token of %s" % (t, a.chars))
    try:
        pp, n, n_oov = ctc_fast.word_lm_perplexity([[chars[t] for t in toks] for toks in lines], lex, eos=not a.no_eos)
    finally:
        lex.close()
    print("word perplexity %.4f, %d terms in %d sentences, %d OOV words" % (pp, n, len(lines), n_oov))
    return pp


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--text", required=True)
    ap.add_argument("--chars", required=True, help="chars.txt: the CTC symbols the device handle maps")
    ap.add_argument("--lm", help="an ARPA character LM, or the .npz of a neural one")
    ap.add_argument("--word-lm", help="an ARPA word LM: word-level perplexity (needs --words)")
    ap.add_argument("--words", help="word list of --word-lm, one per line")
    ap.add_argument("--word-lm-order", type=int, default=2, help="order 2..5 at which --word-lm is read (default 2)")
    ap.add_argument("--space", default="[space]", help="the word separator token of chars.txt (--word-lm)")
    ap.add_argument("--specials", nargs="*", default=[], help="tokens of chars.txt that are whole words (--word-lm)")
    ap.add_argument("--no-eos", action="store_true")
    a = ap.parse_args(argv)
    if bool(a.lm) == bool(a.word_lm) or bool(a.word_lm) != bool(a.words):
        ap.error("one of --lm FILE and --word-lm ARPA --words WORDLIST")
    if a.word_lm:
        return word_perplexity(a)
    chars = {}
    with open(a.chars) as f:
        for line in f:
            tok, i = line.split()
            chars[int(i)] = tok
    if a.lm.endswith(".npz"):
        model = nn_lm.load(a.lm)
        handle = (ctc_fast.DecodeRNNLM if isinstance(model, nn_lm.RNNCharLM) else ctc_fast.DecodeNNLM)(model, chars)

        def word(tok):
            if tok not in model.vocab:
                raise SystemExit("lm_perplexity: the LM does not know the token %r" % tok)
            return model.vocab[tok]
    else:
        model = arpa_lm.ArpaLM(a.lm)
        handle = ctc_fast.DecodeLM(model, chars)
        word = model.word_id
    with open(a.text) as f:
        sents = [[word(t) for t in line.split()] for line in f if line.strip()]
    pp, bpc, n = ctc_fast.lm_perplexity(sents, handle, eos=not a.no_eos)
    print("perplexity %.4f, %.4f bits per character, %d terms in %d sentences" % (pp, bpc, n, len(sents)))
    handle.close()
    return pp


if __name__ == "__main__":
    main()
