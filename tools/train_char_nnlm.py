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

``--rnn --hidden H`` fits the recurrent model of DESIGN.md §4.10 (nn_lm.RNNCharLM) instead: back-
propagation through time over ``<s> sentence </s>``, every position of ``sentence </s>`` predicted
from the state that ``<s>`` and the tokens before it leave.
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


def sentences(lm_tokens, lines):
    """(inputs, targets) per sentence for the recurrent model: <s> + ids predicts ids + </s>"""
    vocab = {t: i for i, t in enumerate(lm_tokens)}
    bos, eos = vocab["<s>"], vocab["</s>"]
    out = []
    for line in lines:
        ids = [vocab[t] for t in line.split()]
        out.append((np.asarray([bos] + ids, dtype=np.int64), np.asarray(ids + [eos], dtype=np.int64)))
    return out


def train_rnn(text, chars, hidden=1024, steps=2000, batch=256, lr=1e-3, seed=0, log=None):
    """the recurrent model h' = relu(bh + Wx[:, id] + Wh h), z = Wo h' + bo: Adam on the cross-entropy
    of whole sentences, ``batch`` sentences per step, padded to the longest and masked"""
    import torch
    with open(chars) as f:
        toks = [l.split()[0] for l in f if l.strip()]
    tokens = list(nn_lm.SPECIALS) + toks
    with open(text) as f:
        lines = [l.strip() for l in f if l.strip()]
    data = sentences(tokens, lines)
    if not data:
        raise ValueError("train_char_nnlm: no training example in %s" % text)
    V, H = len(tokens), int(hidden)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    torch.manual_seed(seed)
    net = torch.nn.RNN(V, H, nonlinearity="relu", batch_first=True).to(dev)
    out = torch.nn.Linear(H, V).to(dev)
    params = list(net.parameters()) + list(out.parameters())
    opt = torch.optim.Adam(params, lr=lr)
    gen = torch.Generator().manual_seed(seed)
    for step in range(steps):
        pick = torch.randint(0, len(data), (min(batch, len(data)),), generator=gen).tolist()
        L = max(data[i][0].shape[0] for i in pick)
        X = np.zeros((len(pick), L), dtype=np.int64)
        Y = np.full((len(pick), L), -100, dtype=np.int64)
        for r, i in enumerate(pick):
            x, y = data[i]
            X[r, :x.shape[0]] = x
            Y[r, :y.shape[0]] = y
        x = torch.nn.functional.one_hot(torch.from_numpy(X).to(dev), V).float()
        h, _ = net(x)
        loss = torch.nn.functional.cross_entropy(out(h).reshape(-1, V), torch.from_numpy(Y).to(dev).reshape(-1),
                                                 ignore_index=-100)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
        if log and (step % 100 == 0 or step == steps - 1):
            log("step %d: %.4f nats per token" % (step, loss.item()))
    g = lambda t: t.detach().cpu().numpy()
    return nn_lm.RNNCharLM(tokens, g(net.weight_ih_l0), g(net.weight_hh_l0), g(net.bias_ih_l0) + g(net.bias_hh_l0),
                           g(out.weight), g(out.bias))


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
    ap.add_argument("--rnn", action="store_true", help="the recurrent model of DESIGN.md §4.10; --hidden takes one width")
    a = ap.parse_args(argv)
    if a.rnn:
        if len(a.hidden) != 1:
            ap.error("--rnn takes one --hidden width")
        lm = train_rnn(a.text, a.chars, a.hidden[0], a.steps, a.batch, a.lr, a.seed, log=print)
        lm.save(a.out)
        print("wrote %s: recurrent, V %d, H %d" % (a.out, lm.V, lm.H))
        return
    lm = train(a.text, a.chars, a.context, a.hidden, a.steps, a.batch, a.lr, a.seed, log=print)
    lm.save(a.out)
    print("wrote %s: V %d, K %d, hidden %s" % (a.out, lm.V, lm.context, a.hidden))


if __name__ == "__main__":
    main()
