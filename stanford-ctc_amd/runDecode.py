"""Decode a likelihood shard (the flow of the reference's ctc_fast/new_decoder/test_simple.py
and runDecode.py:41-77): read ``loglikelihoods_N.pk`` (writeLikelihoods.py), ``chars.txt``,
the alignment file and an ARPA character LM; decode every utterance with the prefix beam
search on the GPU, in batches; write one hypothesis per line and report the character error
rate against the alignments (Wagner-Fischer on the host).

    python runDecode.py --likelihoods loglikelihoods_1.pk --chars chars.txt --alis alis1.txt \\
        --lm text_char.2g.arpa --out hyps.txt [--beam 40 --alpha 1.0 --beta 0.0 --batch 256]

``--method bg`` decodes to words instead (the reference's ``decoder_utils.decode(..., method='bg')``,
ctc_fast/decoder/bg_decoder.pyx): a word list constrains the spellings, an ARPA word-bigram LM
scores every finished word, hypotheses are written as words, and the word error rate is reported
next to the character error rate (reference words: the alignment split at the space symbol).

    python runDecode.py --method bg --likelihoods loglikelihoods_1.pk --chars chars.txt --alis alis1.txt \\
        --words wordlist --word-lm text_word.2g.arpa --out hyps.txt [--specials [noise] [laughter]]
"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from new_decoder import decoder  # noqa: E402
from decoder import decoder_utils  # noqa: E402


def edit_distance(ref, hyp):
    """Levenshtein distance between two sequences"""
    prev = list(range(len(hyp) + 1))
    for i in range(1, len(ref) + 1):
        cur = [i] + [0] * len(hyp)
        for j in range(1, len(hyp) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ref[i - 1] != hyp[j - 1]))
        prev = cur
    return prev[-1]


def load_alis(ali_file, char_file):
    """key -> list of tokens (test_simple.py:13-26; symbol 0 is the blank)"""
    with open(char_file) as f:
        phone_list = [l.rstrip().split()[0] for l in f if l.strip()]
    phone_list.insert(0, "_")
    out = {}
    with open(ali_file) as f:
        for l in f:
            s = l.rstrip().split()
            if s:
                out[s[0]] = [phone_list[int(x)] for x in s[1:]]
    return out


def tokens(hyp, char_int_map):
    """the decoder's string back to tokens (greedy longest match)"""
    toks, pos = [], 0
    by_len = sorted(char_int_map, key=len, reverse=True)
    while pos < len(hyp):
        for t in by_len:
            if hyp.startswith(t, pos):
                toks.append(t)
                pos += len(t)
                break
        else:
            toks.append(hyp[pos])
            pos += 1
    return toks


def decode_bg(a, ll):
    """--method bg: (CER, WER) of the lexicon-constrained word-bigram search"""
    import ctc_fast
    chars = decoder_utils.load_chars(a.chars)
    alis = load_alis(a.alis, a.chars)
    lex = ctc_fast.DecodeLexicon(a.words, chars, a.word_lm, a.space, specials=a.specials)
    keys = sorted(ll)
    errs = n_ref = werrs = n_words = 0
    with open(a.out, "w") as out:
        for g in range(0, len(keys), a.batch):
            ks = keys[g:g + a.batch]
            hyps, scores = ctc_fast.decode_lexicon_beam_batch([np.asarray(ll[k]) for k in ks], lexicon=lex,
                                                              beam=a.beam, alpha=a.alpha, beta=a.beta)
            for k, ids, score in zip(ks, hyps, scores):
                toks = decoder_utils.int_to_char(ids, chars)
                out.write("%s %.6f %s\n" % (k, score, decoder_utils.collapse_seq(toks, a.space)))
                if k in alis:
                    errs += edit_distance(alis[k], toks)
                    n_ref += len(alis[k])
                    ref_words = decoder_utils.collapse_seq(alis[k], a.space).split()
                    werrs += edit_distance(ref_words, decoder_utils.collapse_seq(toks, a.space).split())
                    n_words += len(ref_words)
    cer = errs / float(max(n_ref, 1))
    wer = werrs / float(max(n_words, 1))
    print("decoded %d utterances, CER %.4f (%d / %d), WER %.4f (%d / %d)"
          % (len(keys), cer, errs, n_ref, wer, werrs, n_words))
    return cer, wer


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--likelihoods", required=True)
    ap.add_argument("--chars", required=True)
    ap.add_argument("--alis", required=True)
    ap.add_argument("--lm", help="ARPA character LM (the default method)")
    ap.add_argument("--method", choices=("char", "bg"), default="char",
                    help="char: character LM (default); bg: word list and word-bigram LM")
    ap.add_argument("--words", help="word list, one per line (--method bg)")
    ap.add_argument("--word-lm", help="ARPA word-bigram LM (--method bg)")
    ap.add_argument("--specials", nargs="*", default=[], help="tokens of chars.txt that are whole words")
    ap.add_argument("--space", default="[space]", help="the word separator token of chars.txt")
    ap.add_argument("--out", required=True)
    ap.add_argument("--beam", type=int, default=40)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args(argv)
    with open(a.likelihoods, "rb") as f:
        ll = pickle.load(f)
    if a.method == "bg":
        if not a.words or not a.word_lm:
            ap.error("--method bg needs --words and --word-lm")
        return decode_bg(a, ll)
    if not a.lm:
        ap.error("--lm is required")
    alis = load_alis(a.alis, a.chars)
    dec = decoder.BeamLMDecoder()
    dec.load_chars(a.chars)
    dec.load_lm(a.lm)
    keys = sorted(ll)
    errs = n_ref = 0
    with open(a.out, "w") as out:
        for g in range(0, len(keys), a.batch):
            ks = keys[g:g + a.batch]
            res = dec.decode_batch([np.asfortranarray(ll[k], dtype=np.float64) for k in ks],
                                   a.beam, a.alpha, a.beta)
            for k, (hyp, score) in zip(ks, res):
                out.write("%s %.6f %s\n" % (k, score, hyp))
                if k in alis:
                    errs += edit_distance(alis[k], tokens(hyp, dec.char_int_map))
                    n_ref += len(alis[k])
    cer = errs / float(max(n_ref, 1))
    print("decoded %d utterances, CER %.4f (%d / %d)" % (len(keys), cer, errs, n_ref))
    return cer


if __name__ == "__main__":
    main()
