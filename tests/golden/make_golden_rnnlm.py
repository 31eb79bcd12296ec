"""Draws tests/golden/lm_char_rnn.npz, the recurrent character LM fixture of the decoder tests
(DESIGN.md §4.10), from a seed: the vocabulary is <null> <s> </s> and the 34 tokens of chars.txt
(V = 37), H = 64, Wh scaled to the spectral norm 0.9, the other weights as
tests/rnn_lm_model.random_lm draws them so that the rows span many decades.  About 40 KB.

    python tests/golden/make_golden_rnnlm.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

from tests import rnn_lm_model  # noqa: E402

SEED, HIDDEN, SCALE, RHO = 20241, 64, 1.5, 0.9


def main():
    with open(os.path.join(HERE, "chars.txt")) as f:
        chars = [l.split()[0] for l in f if l.strip()]
    lm = rnn_lm_model.random_lm(SEED, len(chars) + 3, HIDDEN, scale=SCALE, rho=RHO, chars=chars)
    out = os.path.join(HERE, "lm_char_rnn.npz")
    lm.save(out)
    print("%s: V %d, H %d, |Wh|_2 %.3f, %d bytes" % (out, lm.V, lm.H, rnn_lm_model.spectral_norm(lm.Wh),
                                                     os.path.getsize(out)))


if __name__ == "__main__":
    main()
