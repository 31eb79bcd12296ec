"""Draws tests/golden/lm_char_nn.npz, the neural character LM fixture of the decoder tests
(DESIGN.md §4.7), from a seed: the vocabulary is <null> <s> </s> and the 34 tokens of chars.txt
(V = 37), the context K = 8, two hidden layers of 64, weights N(0, 1.5^2 * 2 / fan_in) so that the rows
span many decades.  About 100 KB.

    python tests/golden/make_golden_nnlm.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

from tests import nn_lm_model  # noqa: E402

SEED, CONTEXT, HIDDEN, SCALE = 20240, 8, (64, 64), 1.5


def main():
    with open(os.path.join(HERE, "chars.txt")) as f:
        chars = [l.split()[0] for l in f if l.strip()]
    lm = nn_lm_model.random_lm(SEED, len(chars) + 3, CONTEXT, HIDDEN, scale=SCALE, chars=chars)
    out = os.path.join(HERE, "lm_char_nn.npz")
    lm.save(out)
    print("%s: V %d, K %d, hidden %s, %d bytes" % (out, lm.V, lm.context, list(HIDDEN), os.path.getsize(out)))


if __name__ == "__main__":
    main()
