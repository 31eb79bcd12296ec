"""Bit equality of the prefix beam searches between two builds of the library (DESIGN.md §4.5,
§4.6, §4.6b, §4.7, §4.10).  One run decodes seeded inputs through ctc_fast with the library SCTC_LIB_PATH
names (default: the tree's own) and writes every result to an .npz; --compare requires two such files
to hold the same arrays, byte for byte.  A search that only one of the files has is a difference,
unless --allow-missing names it (a build older than the search cannot have it): then it is named and
not compared.

    SCTC_LIB_PATH=/path/to/parent/libsctc_hip.so python tools/decode_ab.py parent.npz
    python tools/decode_ab.py new.npz
    python tools/decode_ab.py --compare parent.npz new.npz [--allow-missing lexng]

Each run is a process of its own: a process loads one library.  The inputs are small and reach every
path: A = 35 with the LM fixtures of tests/golden (lm_char_5g.arpa, words_bg.txt + lm_word_2g.arpa,
the same lexicon with lm_word_4g.arpa at order 4, lm_char_nn.npz, lm_char_rnn.npz), the character search also without an LM, beams 1, 24 and 150, nbest 1
and 3, a batch of T = 0, 1, 7, 61 and 220 frames, float32 and float64 input, alpha 0 and 0.8.  Per case
the file holds the ids, lengths and scores of every hypothesis and the workspace bytes the entry point
asks for.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stanford-ctc_amd")]
GOLDEN = os.path.join(ROOT, "tests", "golden")

from tests.beam_trace import logsoftmax, peaked  # noqa: E402

A, SPACE = 35, 1
FRAMES = (0, 1, 7, 61, 220)
BEAMS = (1, 24, 150)
BETA = 0.37


def word_input(rs, T, chars, words):
    """beam_trace.peaked over a path that spells lexicon words, so that the lexicon search keeps a full beam"""
    path = []
    while len(path) < T:
        for s in [chars[ch] for ch in words[rs.randint(len(words))]] + [SPACE]:
            if (path and path[-1] == s) or rs.rand() < 0.25:
                path += [0] * rs.randint(1, 3)
            path += [s] * rs.randint(1, 4)
    x = 1.5 * rs.randn(A, T)
    x[np.array(path[:T], dtype=np.int64), np.arange(T)] += 6.0
    return logsoftmax(x)


def providers():
    """{search: (LM object or None, decode function, workspace-bytes function of a config's head and tail)}"""
    import _sctc
    import ctc_fast
    from decoder import decoder_utils, lm as lm_mod
    L = _sctc.lib()
    chars = decoder_utils.load_chars(os.path.join(GOLDEN, "chars.txt"))
    int_char = {v: k for k, v in chars.items()}
    words = decoder_utils.load_words(os.path.join(GOLDEN, "words_bg.txt"))
    lex = ctc_fast.DecodeLexicon(words, {k: v for k, v in chars.items() if v < A},
                                 lm_mod.LM(os.path.join(GOLDEN, "lm_word_2g.arpa")), "[space]",
                                 specials=["[laughter]", "[noise]", "[vocalized-noise]"], A=A)
    lexng = ctc_fast.DecodeLexicon(words, {k: v for k, v in chars.items() if v < A},
                                   os.path.join(GOLDEN, "lm_word_4g.arpa"), "[space]",
                                   specials=["[laughter]", "[noise]", "[vocalized-noise]"], A=A, order=4)

    def with_map(config, name):
        def nbytes(lm, head, tail):
            sw = np.ascontiguousarray(lm.sym_words[:A] if lm is not None else np.zeros(A, np.int32), dtype=np.int32)
            cfg = config(*(head + (0,) + tail + (lm.handle if lm is not None else None, _sctc.i32(sw))))
            return getattr(L, "sctc_ctc_%s_workspace_bytes" % name)(ctypes.byref(cfg))
        return nbytes

    def lex_bytes(lm, head, tail):
        cfg = _sctc.LexBeamConfig(*(head + (lm.space,) + tail + (lm.handle,)))
        return L.sctc_ctc_lexbeam_workspace_bytes(ctypes.byref(cfg))

    def chars_decode(lm, utts, **kw):
        return ctc_fast.decode_beam_batch(utts, lm=lm, **kw)

    def lex_decode(lm, utts, **kw):
        return ctc_fast.decode_lexicon_beam_batch(utts, lexicon=lm, **kw)

    ngram = with_map(_sctc.BeamConfig, "beam")
    out = {
        "nolm": (None, chars_decode, ngram),
        "5g": (ctc_fast.DecodeLM(os.path.join(GOLDEN, "lm_char_5g.arpa"), int_char, A), chars_decode, ngram),
        "lex": (lex, lex_decode, lex_bytes),
        "lexng": (lexng, lex_decode, lex_bytes),
        "nn": (ctc_fast.DecodeNNLM(os.path.join(GOLDEN, "lm_char_nn.npz"), int_char, A), chars_decode,
               with_map(_sctc.NNBeamConfig, "nnbeam")),
        "rnn": (ctc_fast.DecodeRNNLM(os.path.join(GOLDEN, "lm_char_rnn.npz"), int_char, A), chars_decode,
                with_map(_sctc.RNNBeamConfig, "rnnbeam")),
    }
    return out, chars, words


def run(path):
    import _sctc
    searches, chars, words = providers()
    rs = np.random.RandomState(2024)
    inputs = {False: [peaked(rs, A, T) for T in FRAMES], True: [word_input(rs, T, chars, words) for T in FRAMES]}
    Tb = np.ascontiguousarray(FRAMES, dtype=np.int32)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(FRAMES)[:-1]]), dtype=np.int64)
    out = {}
    for search, (lm, decode, nbytes) in searches.items():
        for beam in BEAMS:
            for nbest in (1, 3):
                if nbest > beam:
                    continue
                for dt in (np.float32, np.float64):
                    for alpha in (0.0, 0.8):
                        utts = [u.astype(dt) for u in inputs[search.startswith("lex")]]
                        hyps, scores = decode(lm, utts, beam=beam, alpha=alpha, beta=BETA, nbest=nbest)
                        flat = [h for hs in hyps for h in (hs if nbest > 1 else [hs])]
                        key = "%s/beam%d/nbest%d/%s/alpha%g" % (search, beam, nbest, np.dtype(dt).name, alpha)
                        out[key + "/ids"] = np.concatenate(flat + [np.zeros(0, np.int32)]).astype(np.int32)
                        out[key + "/lengths"] = np.array([len(h) for h in flat], dtype=np.int32)
                        out[key + "/scores"] = np.asarray(scores, dtype=np.float64).reshape(-1)
                        head = (len(FRAMES), A, _sctc.F64 if dt == np.float64 else _sctc.F32, beam, nbest)
                        out[key + "/workspace_bytes"] = np.array(
                            [nbytes(lm, head, (A, _sctc.i32(Tb), _sctc.i64(off), alpha, BETA))], dtype=np.int64)
    np.savez(path, **out)
    longest = max(int(v.max()) for k, v in out.items() if k.endswith("/lengths"))
    print("decode_ab: %d cases from %s -> %s (longest hypothesis %d symbols)"
          % (len(out) // 4, _sctc.LIB_PATH, path, longest))


def compare(pa, pb, allow_missing=()):
    a, b = np.load(pa), np.load(pb)
    searches = [set(k.split("/")[0] for k in z.files) for z in (a, b)]
    for path, mine, theirs in ((pa, searches[0], searches[1]), (pb, searches[1], searches[0])):
        for name in sorted((mine - theirs) & set(allow_missing)):
            print("decode_ab: only %s has the search %s: not compared" % (path, name))
    common = (searches[0] | searches[1]) - ((searches[0] ^ searches[1]) & set(allow_missing))
    files = [set(k for k in z.files if k.split("/")[0] in common) for z in (a, b)]
    bad = sorted(files[0] ^ files[1])
    for k in sorted(files[0] & files[1]):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    for k in bad[:20]:
        print("decode_ab: differs: %s" % k)
    print("decode_ab: %d arrays of %d searches compared, %d differ" % (len(files[0] | files[1]), len(common), len(bad)))
    return 1 if bad or not common else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="the .npz to write")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("--allow-missing", nargs="*", default=[], metavar="SEARCH",
                    help="with --compare: searches that one of the two files may lack")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, allow_missing=a.allow_missing))
    if not a.out:
        ap.error("name the .npz to write, or --compare two")
    run(a.out)


if __name__ == "__main__":
    main()
