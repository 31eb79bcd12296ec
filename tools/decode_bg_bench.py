"""Lexicon-constrained word-bigram decoder throughput: 256 utterances of
T = 1000 frames, A = 35, float32 log-probabilities on the device, beam 40 and 150, a synthetic
lexicon of about 20 000 words with a word bigram.  The yardstick runs in the same process,
alternating: the character decoder with the 5-gram character LM fixture on the same input, once
before and once after the lexicon decoder -- the difference of its two repeats is the run-to-run
spread the comparison is read against.  One JSON line per measurement: median wall time of the
decode call over --reps repeats after a warm-up (hipEvents around the C entry point, descriptor
upload included), utterances/s, workspace and lexicon bytes.  Kernel times: run under
``rocprofv3 --kernel-trace --stats -- python tools/decode_bg_bench.py``.

``--order N`` (3..5) adds two legs between the bigram leg and the second yardstick: the
bigram file itself through the n-gram kernel at order 2 -- the same values and the same single probe per
new word end, so what it adds to the bigram leg is the kernel's larger per-entry state -- and the same
lexicon with a synthetic N-gram word LM: the bigram file's sections, and per higher order 60 000 n-grams
that extend listed ones, three in four so that their suffix is listed too.

    python tools/decode_bg_bench.py [--utts 256] [--frames 1000] [--reps 3] [--words 22600] [--order 4]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import _sctc  # noqa: E402
import arpa_lm  # noqa: E402
import ctc_fast  # noqa: E402
from decoder import decoder_utils, lm as lm_mod, ngram_lm  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SPACE = 1


def synthetic_lexicon(rs, chars, draws, tmp):
    """(words, LM) of random spellings over the single-letter tokens and a random word bigram"""
    letters = [k for k, v in chars.items() if len(k) == 1 and k != "&"]
    words = sorted(set("".join(rs.choice(letters, size=rs.randint(2, 10))) for _ in range(draws)))
    rs.shuffle(words)
    vocab = ["<s>", "</s>", "<UNK>", "[noise]"] + words[:-200]
    lines = ["\\data\\", "ngram 1=%d" % len(vocab), "ngram 2=60000", "", "\\1-grams:"]
    for w in vocab:
        lines.append("%.6f\t%s\t%.6f" % (-99.0 if w == "<s>" else -(1 + 4 * rs.rand()), w, -(0.1 + rs.rand())))
    lines += ["", "\\2-grams:"]
    pairs = set()
    while len(pairs) < 60000:
        pairs.add((0 if rs.rand() < 0.05 else rs.randint(2, len(vocab)), rs.randint(1, len(vocab))))
    for a, b in sorted(pairs):
        lines.append("%.6f\t%s %s" % (-(0.1 + 3 * rs.rand()), vocab[a], vocab[b]))
    lines += ["", "\\end\\", ""]
    path = os.path.join(tmp, "words.arpa")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return words, lm_mod.LM(path), (vocab, sorted(pairs), lines[:-3])


def synthetic_ngram(rs, parts, order, tmp, per_order=60000):
    """the NgramLM of the bigram file's sections plus ``per_order`` n-grams of every order 3..order, each
    the extension of a listed one (so every prefix is listed)"""
    vocab, pairs, lines = parts
    lines = list(lines)
    lines[2:3] = ["ngram 2=%d" % len(pairs)] + ["ngram %d=%d" % (n, per_order) for n in range(3, order + 1)]
    # the back-off column the bigrams lack in the bigram file
    first = lines.index("\\2-grams:") + 1
    for i in range(first, first + len(pairs)):
        lines[i] += "\t%.6f" % -(0.1 + rs.rand())
    prev = pairs
    follow = {}
    for g in prev:
        follow.setdefault(g[:-1], []).append(g[-1])
    for n in range(3, order + 1):
        grams = set()
        while len(grams) < per_order:
            g = prev[rs.randint(len(prev))]
            nxt = follow.get(g[1:])
            c = nxt[rs.randint(len(nxt))] if nxt and rs.rand() < 0.75 else rs.randint(1, len(vocab))
            grams.add(g + (int(c),))
        prev = sorted(grams)
        for g in prev:
            follow.setdefault(g[:-1], []).append(g[-1])
        lines += ["", "\\%d-grams:" % n]
        for g in prev:
            lines.append("%.6f\t%s" % (-(0.1 + 3 * rs.rand()), " ".join(vocab[i] for i in g))
                         + ("" if n == order else "\t%.6f" % -(0.1 + rs.rand())))
    lines += ["", "\\end\\", ""]
    path = os.path.join(tmp, "words_%dg.arpa" % order)
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return ngram_lm.NgramLM(path, order)


def posteriors(rs, A, T, chars, words):
    """peaked on a random word sequence: runs of 1..3 frames, blanks between equal neighbours"""
    path = []
    while len(path) < T:
        for s in [chars[ch] for ch in words[rs.randint(len(words))]] + [SPACE]:
            if (path and path[-1] == s) or rs.rand() < 0.25:
                path += [0] * rs.randint(1, 3)
            path += [s] * rs.randint(1, 4)
    x = 1.5 * rs.randn(A, T)
    x[np.array(path[:T]), np.arange(T)] += 4.0
    m = x.max(axis=0, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))).astype(np.float32)


def timed(torch, run, reps):
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--words", type=int, default=22600, help="random spellings drawn (duplicates drop out)")
    ap.add_argument("--order", type=int, default=2, help="3..5: also time the lexicon with a synthetic N-gram word LM")
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    A, B, T = 35, a.utts, a.frames
    rs = np.random.RandomState(0)
    chars = decoder_utils.load_chars(os.path.join(GOLDEN, "chars.txt"))
    with tempfile.TemporaryDirectory() as tmp:
        words, wlm, parts = synthetic_lexicon(rs, chars, a.words, tmp)
        nlm = synthetic_ngram(np.random.RandomState(a.order), parts, a.order, tmp) if a.order > 2 else None
        lm2 = ngram_lm.NgramLM(os.path.join(tmp, "words.arpa"), 2) if a.order > 2 else None
    lex = ctc_fast.DecodeLexicon(words, chars, wlm, "[space]", specials=["[laughter]", "[noise]"], A=A)
    nlex = ctc_fast.DecodeLexicon(words, chars, nlm, "[space]", specials=["[laughter]", "[noise]"], A=A) if nlm else None
    lex2 = ctc_fast.DecodeLexicon(words, chars, lm2, "[space]", specials=["[laughter]", "[noise]"], A=A) if lm2 else None
    clm = ctc_fast.DecodeLM(arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_5g.arpa")),
                            {v: k for k, v in chars.items()}, A)
    rows = np.concatenate([posteriors(rs, A, T, chars, words).T for _ in range(B)], axis=0)
    dev = torch.from_numpy(rows).cuda()
    Tb = np.full(B, T, dtype=np.int32)
    off = np.arange(B, dtype=np.int64) * T
    sw = np.ascontiguousarray(clm.sym_words, dtype=np.int32)
    ids = torch.empty(B * T, dtype=torch.int32, device="cuda")
    lens = torch.empty(B, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, dtype=torch.float64, device="cuda")
    for beam in (40, 150):
        ccfg = _sctc.BeamConfig(B, A, _sctc.F32, beam, 1, 0, A, _sctc.i32(Tb), _sctc.i64(off), 1.0, 0.5,
                                clm.handle, _sctc.i32(sw))
        lcfg = _sctc.LexBeamConfig(B, A, _sctc.F32, beam, 1, lex.space, A, _sctc.i32(Tb), _sctc.i64(off), 1.0, 0.5,
                                   lex.handle)
        ncfg = _sctc.LexBeamConfig(B, A, _sctc.F32, beam, 1, lex.space, A, _sctc.i32(Tb), _sctc.i64(off), 1.0, 0.5,
                                   nlex.handle) if nlex else None
        cfg2 = _sctc.LexBeamConfig(B, A, _sctc.F32, beam, 1, lex.space, A, _sctc.i32(Tb), _sctc.i64(off), 1.0, 0.5,
                                   lex2.handle) if lex2 else None
        cbytes = L.sctc_ctc_beam_workspace_bytes(ctypes.byref(ccfg))
        lbytes = L.sctc_ctc_lexbeam_workspace_bytes(ctypes.byref(lcfg))
        ws = torch.empty(max(cbytes, lbytes), dtype=torch.uint8, device="cuda")

        def run_char():
            _sctc.check(L.sctc_ctc_beam_decode_batch(ctypes.byref(ccfg), dev.data_ptr(), ids.data_ptr(),
                                                     lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), cbytes,
                                                     _sctc.current_stream_ptr()), "decode")

        def run_lex():
            _sctc.check(L.sctc_ctc_lexbeam_decode_batch(ctypes.byref(lcfg), dev.data_ptr(), ids.data_ptr(),
                                                        lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), lbytes,
                                                        _sctc.current_stream_ptr()), "decode")

        def run_ng():
            _sctc.check(L.sctc_ctc_lexbeam_decode_batch(ctypes.byref(ncfg), dev.data_ptr(), ids.data_ptr(),
                                                        lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), lbytes,
                                                        _sctc.current_stream_ptr()), "decode")

        def run_ng2():
            _sctc.check(L.sctc_ctc_lexbeam_decode_batch(ctypes.byref(cfg2), dev.data_ptr(), ids.data_ptr(),
                                                        lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), lbytes,
                                                        _sctc.current_stream_ptr()), "decode")
        legs = [("char 5-gram (yardstick)", run_char, cbytes, None), ("lexicon bigram", run_lex, lbytes, lex)]
        if nlex:
            legs.append(("lexicon bigram file, n-gram kernel at order 2", run_ng2, lbytes, lex2))
            assert L.sctc_ctc_lexbeam_workspace_bytes(ctypes.byref(ncfg)) == lbytes
            legs.append(("lexicon %d-gram" % a.order, run_ng, lbytes, nlex))
        legs.append(legs[0])
        for what, run, nbytes, handle in legs:
            t = timed(torch, run, a.reps)
            print(json.dumps({"decoder": what, "beam": beam, "utts": B, "frames": T, "A": A, "seconds": round(t, 4),
                              "utts_per_s": round(B / t, 1), "us_per_frame": round(t * 1e6 / T, 2),
                              "workspace_mb": round(nbytes / 2 ** 20, 1),
                              "lexicon_mb": round(handle.device_bytes / 2 ** 20, 2) if handle else None,
                              "words": len(words), "nodes": lex.nodes, "mean_len": float(lens.float().mean()),
                              "score0": float(scores[0])}), flush=True)
        del ws


if __name__ == "__main__":
    main()
