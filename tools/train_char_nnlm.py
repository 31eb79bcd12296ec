#!/usr/bin/env python3
"""Fits the feed-forward character LM of DESIGN.md §4.7 (stanford-ctc_amd/nn_lm.py) to a text file
and writes the ``.npz`` the decoder loads (``runDecode.py --lm model.npz``).

The text holds one sentence per line, space-separated character tokens as in chars.txt (``[space]``
for the word separator).  Every position of ``sentence </s>`` is one training example: the window
of the K tokens before it, padded as the decoder pads it (``<null>`` .. ``<s>`` + prefix), predicts
the token.  Plain PyTorch (Adam on the cross-entropy), on the GPU when there is one: plumbing, the
decoder's kernels are not involved.

    python tools/train_char_nnlm.py --text text_char.txt --chars chars.txt --out lm.npz \\
        [--context 19 --hidden 1024 1024 --steps 2000 --batch 256 --lr 1e-3 --seed 0]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stanford-ctc_amd")]

import nn_lm  # noqa: E402


def examples(lm_tokens, context, lines):
    """(windows int64 [n, K], targets int64 [n]) of the sentences, padded as NNCharLM.context_ids"""
    vocab = {t: i for i, t in enumerate(lm_tokens)}
    null, bos, eos = vocab["<null>"], vocab["<s>"], vocab["</s>"]
    X, Y = [], []
    for line in lines:
        ids = [vocab[t] for t in line.split()]
        seq = [null] * (context - 1) + [bos] + ids + [eos]
        for i in range(len(ids) + 1):
            X.append(seq[i:i + context])
            Y.append(seq[i + context])
    return np.asarray(X, dtype=np.int64).reshape(-1, context), np.asarray(Y, dtype=np.int64)


def train(text, chars, context=19, hidden=(1024, 1024), steps=2000, batch=256, lr=1e-3, seed=0, log=None):
    import torch
    with open(chars) as f:
        toks = [l.split()[0] for l in f if l.strip()]
    tokens = list(nn_lm.SPECIALS) + toks
    with open(text) as f:
        lines = [l.strip() for l in f if l.strip()]
    X, Y = examples(tokens, context, lines)
    if X.shape[0] == 0:
        raise ValueError("train_char_nnlm: no training example in %s" % text)
    V = len(tokens)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    torch.manual_seed(seed)
    widths = [context * V] + list(hidden) + [V]
    layers = []
    for l in range(len(widths) - 1):
        layers.append(torch.nn.Linear(widths[l], widths[l + 1]))
        if l < len(widths) - 2:
            layers.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    gen = torch.Generator().manual_seed(seed)
    for step in range(steps):
        pick = torch.randint(0, X.shape[0], (min(batch, X.shape[0]),), generator=gen).to(dev)
        x = torch.nn.functional.one_hot(Xd[pick], V).reshape(pick.shape[0], -1).float()
        loss = torch.nn.functional.cross_entropy(net(x), Yd[pick])
        opt.zero_grad()
        loss.backward()
        opt.step()
        if log and (step % 100 == 0 or step == steps - 1):
            log("step %d: %.4f nats per token" % (step, loss.item()))
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    return nn_lm.NNCharLM(tokens, context, [m.weight.detach().cpu().numpy() for m in lin],
                          [m.bias.detach().cpu().numpy() for m in lin])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--text", required=True)
    ap.add_argument("--chars", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--context", type=int, default=19)
    ap.add_argument("--hidden", type=int, nargs="+", default=[1024, 1024])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    lm = train(a.text, a.chars, a.context, a.hidden, a.steps, a.batch, a.lr, a.seed, log=print)
    lm.save(a.out)
    print("wrote %s: V %d, K %d, hidden %s" % (a.out, lm.V, lm.context, a.hidden))


if __name__ == "__main__":
    main()
