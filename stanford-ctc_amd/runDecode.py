"""Decode a likelihood shard (the flow of the reference's ctc_fast/new_decoder/test_simple.py
and runDecode.py:41-77): read ``loglikelihoods_N.pk`` (writeLikelihoods.py), ``chars.txt``,
the alignment file and an ARPA character LM; decode every utterance with the prefix beam
search on the GPU, in batches; write one hypothesis per line and report the character error
rate against the alignments (Wagner-Fischer on the host).

    python runDecode.py --likelihoods loglikelihoods_1.pk --chars chars.txt --alis alis1.txt \\
        --lm text_char.2g.arpa --out hyps.txt [--beam 40 --alpha 1.0 --beta 0.0 --batch 256]
"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from new_decoder import decoder  # noqa: E402


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--likelihoods", required=True)
    ap.add_argument("--chars", required=True)
    ap.add_argument("--alis", required=True)
    ap.add_argument("--lm", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--beam", type=int, default=40)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args(argv)
    with open(a.likelihoods, "rb") as f:
        ll = pickle.load(f)
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
