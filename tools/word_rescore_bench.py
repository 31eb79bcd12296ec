"""The word LM as a second pass, on the device against the host route, on the input of
tools/decode_bench.py: 256 utterances of T = 1000 frames, A = 35, float32 log-probabilities on the device.  The first
pass is the n-gram search (5-gram fixture, beam 40, alpha 1.0, beta 0.5) with nbest = 40, its output left on the
device; the word LM is the golden word list with the 4-gram fixture (tests/golden), read at --order.

One JSON line with, each the median of --reps calls after a warm-up and with max - min as the spread:
  * ``word_score_s``: ctc_fast.word_lm_score_batch on the search's device ids (workspace, descriptors, one launch;
    nothing read back; host clock ending in a synchronise), and ``word_stream_s``: hipEvents around the same call when
    it is queued behind about half a millisecond of other work, so that the host's share of the call is over before
    the stream gets there: the descriptor copy and the kernel, back to back -- the kernel alone to within that copy
    (24 bytes a sequence);
  * ``host_s``: the host route, reading the ids back and ctc_fast.word_lm_sentence_scores, and ``sums_equal``: the two
    routes' sums compared for equal bits;
  * ``rescore_words_s``: ctc_fast.rescore_nbest with the word LM, next to ``rescore_plain_s``: rescore_nbest(lm=None) on
    the same input -- the difference is what the word term adds to the second pass;
  * ``label_bytes``: 4 bytes per symbol of the hypotheses, the bytes the kernel has to read once.
The kernel by name: run under ``rocprofv3 --kernel-trace --stats -- python tools/word_rescore_bench.py --no-host``, in a
run of its own.

    python tools/word_rescore_bench.py [--utts 256] [--frames 1000] [--nbest 40] [--reps 5] [--order 4] [--no-host]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]

import _sctc  # noqa: E402
import ctc_fast  # noqa: E402
from tools import decode_bench  # noqa: E402
from tools.rescore_bench import med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--nbest", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (profiling runs)")
    a = ap.parse_args()
    torch = _sctc.require_gpu()
    A, B, T, K = 35, a.utts, a.frames, a.nbest
    dev, ngram = decode_bench.load_input(torch, B, T, A)
    golden = os.path.join(ROOT, "tests", "golden")
    lex = ctc_fast.DecodeLexicon(os.path.join(golden, "words_bg.txt"), os.path.join(golden, "chars.txt"),
                                 os.path.join(golden, "lm_word_4g.arpa"), "[space]", specials=["[laughter]", "[noise]"],
                                 A=A, order=a.order)
    T_b = [T] * B
    sync = torch.cuda.synchronize
    ids, lens, scores = ctc_fast.decode_beam_batch(dev, T_b, beam=40, alpha=1.0, beta=0.5, lm=ngram, nbest=K, device=True)
    U = lens.cpu().numpy().astype(np.int64)
    off = (K * (np.arange(B, dtype=np.int64) * T)[:, None] + np.arange(K, dtype=np.int64)[None, :] * T).reshape(-1)

    score_s, score_spread = med(lambda: ctc_fast.word_lm_score_batch((ids, U, off), lex, device=True), a.reps, sync)
    ev = []
    ahead = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")       # 1 GiB: a pass over it keeps the stream busy

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ahead.add_(1.0)
        e0.record()
        ctc_fast.word_lm_score_batch((ids, U, off), lex, device=True)
        e1.record()
        ev.append((e0, e1))
    timed()
    sync()
    del ev[:]
    for _ in range(a.reps):
        timed()
        sync()
    kern = [e0.elapsed_time(e1) / 1e3 for e0, e1 in ev]
    d_sums, d_counts, _ = ctc_fast.word_lm_score_batch((ids, U, off), lex)
    host_sums = []

    def host():
        h_ids = ids.cpu().numpy()
        rows = [h_ids[o:o + u] for o, u in zip(off, U)]
        host_sums[:] = [ctc_fast.word_lm_sentence_scores(rows, lex)[0]]
    host_s = host_spread = None
    if not a.no_host:
        host_s, host_spread = med(host, max(1, min(a.reps, 2)), sync)
    plain_s, plain_spread = med(lambda: ctc_fast.rescore_nbest(dev, (ids, lens, scores), lengths=T_b, lm=None, beta=0.5),
                                a.reps, sync)
    words_s, words_spread = med(lambda: ctc_fast.rescore_nbest(dev, (ids, lens, scores), lengths=T_b, lm=None, beta=0.5,
                                                               word_lm=lex, word_alpha=0.5, word_beta=0.5), a.reps, sync)
    order, _ = ctc_fast.rescore_nbest(dev, (ids, lens, scores), lengths=T_b, lm=None, beta=0.5, word_lm=lex, word_alpha=0.5,
                                      word_beta=0.5)
    print(json.dumps({"utts": B, "frames": T, "nbest": K, "order": a.order, "hypotheses": int(B * K),
                      "symbols": int(U.sum()), "label_bytes": int(4 * U.sum()), "words": int(d_counts[:, 0].sum()),
                      "oov_words": int(d_counts[:, 1].sum()), "lexicon_bytes": lex.device_bytes,
                      "word_score_s": round(score_s, 6), "word_score_spread_s": round(score_spread, 6),
                      "word_stream_s": round(float(np.median(kern)), 6), "word_stream_spread_s": round(max(kern) - min(kern), 6),
                      "host_s": host_s and round(host_s, 4), "host_spread_s": host_spread and round(host_spread, 4),
                      "host_over_device": host_s and round(host_s / score_s, 1),
                      "sums_equal": bool(d_sums.tobytes() == host_sums[0].tobytes()) if host_sums else None,
                      "rescore_plain_s": round(plain_s, 5), "rescore_plain_spread_s": round(plain_spread, 5),
                      "rescore_words_s": round(words_s, 5), "rescore_words_spread_s": round(words_spread, 5),
                      "changed_1best": int((order[:, 0] != 0).sum())}), flush=True)
    lex.close()


if __name__ == "__main__":
    main()
