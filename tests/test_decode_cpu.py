"""CPU checks of the prefix beam search decoder: the ARPA reader and the packed
device table against a brute-force back-off scorer, the Python restatement of the search against
the reference's own results (tests/golden/decode_ref.npz, make_golden_decode.py), the new C ABI
entries and the argument errors that need no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import beam_model
from tests.helpers import arpa_backoff as brute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

TOY_ARPA = """
\\data\\
ngram 1=6
ngram 2=5
ngram 3=2

\\1-grams:
-1.0\t</s>
-99\t<s>\t-0.5
-0.7\ta\t-0.3
-0.9\tb
-1.2\tc\t-0.2
-2.0\t<unk>

\\2-grams:
-0.2\t<s> a\t-0.1
-0.4\ta b\t-0.25
-0.3\ta a
-0.5\tc a
-0.6\tb </s>

\\3-grams:
-0.05\t<s> a b
-0.15\ta b </s>

\\end\\
"""


def check_lm(lm, rs, n=300):
    words = list(range(1, len(lm.words) + 1))
    table = lm.pack()
    for g, (p, bo) in lm.ngrams.items():
        got = arpa_lm_mod().lookup_packed(table, arpa_lm_mod().pack_ngram(g))
        assert got is not None and got[0] == p and got[1] == bo, g
    cap = table[0].shape[0]
    assert cap & (cap - 1) == 0 and np.count_nonzero(table[0]) == len(lm.ngrams) <= cap // 2
    for _ in range(n):
        ctx = [lm.bos] + list(rs.choice(words, size=rs.randint(0, 2 * lm.order)))
        w = int(rs.choice(words))
        assert abs(float(lm.score_ids(ctx, w)) - brute(lm, ctx, w)) < 1e-4, (ctx, w)


def arpa_lm_mod():
    import arpa_lm
    return arpa_lm


def test_arpa_reader_toy():
    import arpa_lm
    lm = arpa_lm.ArpaLM(text=TOY_ARPA)
    assert lm.order == 3 and lm.words[:2] == ["</s>", "<s>"]
    a, b, c = (lm.vocab[x] for x in "abc")
    # a missing back-off column reads as 0; a listed n-gram wins
    assert lm.ngrams[(b,)][1] == 0.0 and lm.ngrams[(lm.bos, a)][1] == np.float32(-0.1)
    assert lm.score_ids([lm.bos, a], b) == np.float32(-0.05)
    # back-off chain: bo(<s> a) + p(a a)
    assert lm.score_ids([lm.bos, a], a) == np.float32(np.float32(-0.3) + np.float32(-0.1))
    # unknown tokens score as the file's <unk>, with the context's back-offs
    assert lm.word_id("zz") == lm.unk
    assert lm.score_ids([lm.bos, c], lm.unk) == np.float32(np.float32(-2.0) + np.float32(-0.2))
    # kenlm's full_scores: one entry per word and </s>
    sc = list(lm.full_scores("a b"))
    assert len(sc) == 3 and sc[1][0] == pytest.approx(-0.05) and sc[2][0] == pytest.approx(-0.15)
    check_lm(lm, np.random.RandomState(1))


def test_arpa_default_unk_and_limits():
    import arpa_lm
    lm = arpa_lm.ArpaLM(text=TOY_ARPA.replace("ngram 1=6", "ngram 1=5").replace("-2.0\t<unk>\n", ""))
    assert lm.ngrams[(lm.unk,)] == (np.float32(-100.0), np.float32(0.0))
    with pytest.raises(ValueError):
        arpa_lm.ArpaLM(text=TOY_ARPA.replace("ngram 2=5", "ngram 2=7"))
    nine = "\\data\\\n" + "".join("ngram %d=1\n" % n for n in range(1, 10)) + "\n"
    for n in range(1, 10):
        nine += "\\%d-grams:\n-0.1\t%s\n" % (n, " ".join(["<s>"] * n))
    with pytest.raises(ValueError):
        arpa_lm.ArpaLM(text=nine + "\\end\\\n")
    big = "\\data\\\nngram 1=300\n\n\\1-grams:\n" + "".join("-1\tw%d\n" % i for i in range(299)) + "-99\t<s>\n\\end\\\n"
    with pytest.raises(ValueError):
        arpa_lm.ArpaLM(text=big)


def test_arpa_order8_keys():
    """an order-8 model: 64-bit keys with no free byte, every n-gram found in the packed table"""
    import arpa_lm
    rs = np.random.RandomState(3)
    vocab = ["<s>", "</s>", "<unk>"] + ["w%d" % i for i in range(250)]     # ids up to 253
    lines = {1: ["%.4f\t%s\t%.4f" % (-rs.rand() * 3, w, -rs.rand()) for w in vocab]}
    seqs = [["<s>"] + list(rs.choice(vocab[3:], size=12)) for _ in range(30)]
    for n in range(2, 9):
        gs = sorted({tuple(s[i:i + n]) for s in seqs for i in range(len(s) - n + 1)})
        lines[n] = ["%.4f\t%s%s" % (-rs.rand() * 2, " ".join(g), "" if n == 8 else "\t%.4f" % -rs.rand())
                    for g in gs]
    txt = "\\data\\\n" + "".join("ngram %d=%d\n" % (n, len(lines[n])) for n in lines) + "\n"
    txt += "".join("\\%d-grams:\n%s\n\n" % (n, "\n".join(lines[n])) for n in lines) + "\\end\\\n"
    lm = arpa_lm.ArpaLM(text=txt)
    assert lm.order == 8 and len(lm.words) == 253
    key = arpa_lm.pack_ngram([253, 252, 251, 250, 249, 248, 247, 246])
    assert key >> 56 == 253
    check_lm(lm, rs, n=200)
    # contexts that follow the listed 8-grams exercise the longest matches
    for s in seqs[:10]:
        ids = [lm.vocab[t] for t in s]
        for i in range(1, len(ids)):
            assert abs(float(lm.score_ids(ids[:i], ids[i])) - brute(lm, ids[:i], ids[i])) < 1e-4


@pytest.mark.parametrize("name", ["lm_char_2g.arpa", "lm_char_5g.arpa"])
def test_fixture_lms(name):
    import arpa_lm
    lm = arpa_lm.ArpaLM(os.path.join(GOLDEN, name))
    assert lm.order == (2 if "2g" in name else 5)
    assert os.path.getsize(os.path.join(GOLDEN, name)) < 100 * 1024
    check_lm(lm, np.random.RandomState(5))


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "decode_ref.npz"))
    return z, int(z["n"])


def sym_words(lm, A):
    chars = {}
    with open(os.path.join(GOLDEN, "chars.txt")) as f:
        for l in f:
            t, i = l.split()
            chars[int(i)] = t
    return lm.symbol_words(chars, A)


def test_chars_fixture_has_unknown_symbol():
    import arpa_lm
    for name in ("lm_char_2g.arpa", "lm_char_5g.arpa"):
        lm = arpa_lm.ArpaLM(os.path.join(GOLDEN, name))
        sw = sym_words(lm, 35)
        assert (sw[1:] == lm.unk).sum() >= 1 and sw[4] == lm.unk


def test_restatement_against_reference():
    """tests/beam_model.py (float32 reads, stable combine, the fixed tie rule) reproduces the
    reference's hypotheses and scores: the yardstick of the GPU tests"""
    import arpa_lm
    z, n = golden_cases()
    lms = {k: arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_%s.arpa" % k)) for k in ("2g", "5g")}
    compared = 0
    for i in range(n):
        A, T, beam, alpha, beta = z["cfg%d" % i]
        A, T, beam = int(A), int(T), int(beam)
        if beam > 40 and T > 30:
            continue                   # the slow ones run on the GPU side only
        lm = lms[str(z["lm%d" % i])]
        (hyp, score), = beam_model.decode(z["lp%d" % i], beam, alpha, beta,
                                          beam_model.arpa_rows(lm, sym_words(lm, A)))
        ref = float(z["score%d" % i])
        assert abs(score - ref) <= 1e-9 * abs(ref) + 1e-12, (i, score, ref)
        if z["margin%d" % i] >= 1e-6:
            assert list(hyp) == list(z["hyp%d" % i]), i
        compared += 1
    assert compared >= 25


def test_restatement_against_reference_truncations():
    """the reference's top entry after EVERY frame (decode_ref_trace.npz: each truncation lp[:, :t]
    decoded by the reference), at alpha / beta that are no float32 numbers, against the model's
    trace.  alpha is handed over as a Python float, as callers do: a model that multiplied
    alpha * LM in float32 misses the 1e-9 here (1.2e-7 relative at alpha 0.8 and 1.3)."""
    import arpa_lm
    z = np.load(os.path.join(GOLDEN, "decode_ref_trace.npz"))
    lms = {k: arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_%s.arpa" % k)) for k in ("2g", "5g")}
    frames = compared = 0
    seen = set()
    for i in range(int(z["n"])):
        A, T, beam = (int(v) for v in z["cfg%d" % i][:3])
        alpha, beta = float(z["cfg%d" % i][3]), float(z["cfg%d" % i][4])
        assert float(np.float32(alpha)) != alpha
        seen.add((A, beam, str(z["lm%d" % i])))
        lm = lms[str(z["lm%d" % i])]
        trace = []
        top = beam_model.decode(z["lp%d" % i], beam, alpha, beta, beam_model.arpa_rows(lm, sym_words(lm, A)),
                                trace=trace)
        assert len(trace) == T and top[0] == trace[-1]["beam"][0]
        ends = np.cumsum(z["len%d" % i])
        for t, fr in enumerate(trace):
            (hyp, score), ref = fr["beam"][0], float(z["score%d" % i][t])
            assert abs(score - ref) <= 1e-9 * abs(ref) + 1e-12, (i, t, alpha, score, ref)
            if len(fr["beam"]) < 2 or score - fr["beam"][1][1] >= 1e-6:
                assert list(hyp) == list(z["hyp%d" % i][ends[t] - z["len%d" % i][t]:ends[t]]), (i, t)
                compared += 1
            frames += 1
    assert frames >= 200 and compared >= 0.9 * frames
    assert {a for a, _, _ in seen} == {8, 35} and {b for _, b, _ in seen} == {16, 40}
    assert os.path.getsize(os.path.join(GOLDEN, "decode_ref_trace.npz")) < 200 * 1024


def test_trace_option_leaves_results_alone():
    rs = np.random.RandomState(3)
    lp = np.log(rs.dirichlet(np.ones(6), size=12).T)
    plain = beam_model.decode(lp, 5, 0.0, 0.4, None, nbest=5)
    trace = []
    assert beam_model.decode(lp, 5, 0.0, 0.4, None, nbest=5, trace=trace) == plain
    assert [e for e in trace[-1]["beam"]] == plain and len(trace) == 12
    assert trace[0]["cut"] is not None and trace[0]["cut"] <= trace[0]["beam"][-1][1]
    assert beam_model.decode(lp[:, :1], 8, 0.0, 0.4, None, trace=trace) and trace[-1]["cut"] is None
    for t in range(1, 12):                     # the beam after frame t is the final beam of lp[:, :t]
        assert beam_model.decode(lp[:, :t], 5, 0.0, 0.4, None, nbest=5) == trace[t - 1]["beam"]


def test_lm_row_read_off_on_the_model():
    """the read-off of tests/test_gpu_decode_trace.py, applied to the model: forced prefixes give
    back the float32 rows, which lie within the float32 summation bound of a float64 back-off"""
    import arpa_lm
    from tests import beam_trace as bt
    lm = arpa_lm.ArpaLM(os.path.join(GOLDEN, "lm_char_5g.arpa"))
    sw = sym_words(lm, 35)
    rs = np.random.RandomState(31)
    prefixes = bt.lm_row_prefixes(lm, sw, rs)[::3]
    rows = []
    for P in prefixes:
        lp = bt.forced_prefix_frames(rs, 35, P)
        res = beam_model.decode(lp, 40, 0.7, 0.0, beam_model.arpa_rows(lm, sw), nbest=40)
        rows.append(bt.recover_lm_row(P, lp, [r[0] for r in res], [r[1] for r in res], 0.7))
    st = bt.check_lm_rows(lm, sw, prefixes, rows, 0.7)
    assert st["pairs"] >= 200 and st["early_break"] and st["full_chain"] and st["single"] >= 20


def test_tie_inputs_hold_their_preconditions():
    """the cheap inputs of the GPU tie tests: the model cuts inside a -inf tie / an exact tie of
    one cell kind often enough, and relies on no tie across cell kinds"""
    from tests import beam_trace as bt
    lp = bt.sparse_frames(np.random.RandomState(2000), 8, 40)
    st = bt.check_model(bt.model_trace(lp, 32, 0.0, 0.4, None), 32, near_cap=0.0)
    assert 2 * st["cut_in_inf_tie"] >= 40
    lp = bt.dead_frame(np.random.RandomState(2101), 8, 40, 12)
    st = bt.check_model(bt.model_trace(lp, 32, 0.0, 0.4, None), 32, near_cap=0.0)
    assert 2 * st["cut_in_inf_tie"] >= 40
    for seed in (0, 2, 4, 7):
        lp = bt.twins(np.random.RandomState(2200 + seed), 7, 40, [(1, 2), (4, 6)])
        st = bt.check_model(bt.model_trace(lp, 12, 0.0, 0.3, None), 12, exact_ties=True)
        assert st["ties"] >= 300 and st["cut_in_tie"] >= 5
    # and a seed whose ties cross cell kinds is refused
    lp = bt.twins(np.random.RandomState(2203), 7, 40, [(1, 2), (4, 6)])
    with pytest.raises(AssertionError):
        bt.check_model(bt.model_trace(lp, 12, 0.0, 0.3, None), 12, exact_ties=True)


def test_restatement_edges():
    lp = np.log(np.full((4, 0), 0.25))
    assert beam_model.decode(lp) == [((), 0.0)]
    lp = np.full((3, 2), -np.inf)
    lp[0] = 0.0
    assert beam_model.decode(lp, beam=4) == [((), 0.0)]


# ---- the C ABI ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sctc():
    import __graft_entry__ as ge
    import _sctc
    if not os.path.exists(_sctc.LIB_PATH):
        ge.build()
    return _sctc


NEW_SYMBOLS = ["sctc_lm_create", "sctc_lm_destroy", "sctc_ctc_beam_workspace_bytes", "sctc_ctc_beam_decode_batch"]


def test_decoder_abi_symbols(sctc):
    src = open(os.path.join(ROOT, "include", "sctc.h")).read()
    L = sctc.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in src
        assert name in sctc.PROTOTYPES
        assert hasattr(L, name)
    assert L.sctc_abi_version() == 6


def test_beam_config_mirror(sctc, tmp_path):
    prog = tmp_path / "bc.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sctc.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(sctc_beam_config), offsetof(sctc_beam_config, ld),'
        ' offsetof(sctc_beam_config, alpha), offsetof(sctc_beam_config, lm), offsetof(sctc_beam_config, sym_word));'
        ' return 0;}\n')
    exe = tmp_path / "bc"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B = sctc.BeamConfig
    assert got == [ctypes.sizeof(B), B.ld.offset, B.alpha.offset, B.lm.offset, B.sym_word.offset]


def beam_cfg(sctc, B=1, A=35, beam=40, nbest=1, T=10, dtype=None, ld=None, alpha=1.0, sym=None):
    T_b = np.full(B, T, dtype=np.int32)
    off = np.arange(B, dtype=np.int64) * max(T, 0)
    keep = (T_b, off)
    cfg = sctc.BeamConfig(B, A, sctc.F32 if dtype is None else dtype, beam, nbest, 0, A if ld is None else ld,
                          sctc.i32(T_b), sctc.i64(off), alpha, 0.0, None,
                          None if sym is None else sctc.i32(sym))
    return cfg, keep


def test_beam_argument_errors_need_no_gpu(sctc):
    L = sctc.lib()
    ws = lambda c: L.sctc_ctc_beam_workspace_bytes(ctypes.byref(c))
    cfg, keep = beam_cfg(sctc)
    n = ws(cfg)
    assert n >= 40 * 35 * 24 + 10 * 40 * 4
    cfg, keep = beam_cfg(sctc, B=3, T=1000, beam=150)
    assert ws(cfg) >= 3 * (150 * 35 * 24 + 1000 * 150 * 4)
    for bad in (dict(beam=0), dict(beam=257), dict(A=257), dict(A=1), dict(nbest=41), dict(nbest=0),
                dict(B=0), dict(T=-1), dict(dtype=7), dict(ld=20), dict(alpha=float("nan"))):
        cfg, keep = beam_cfg(sctc, **bad)
        assert ws(cfg) == 0, bad
        assert L.sctc_ctc_beam_decode_batch(ctypes.byref(cfg), None, None, None, None, None, 0, None) == -1
    cfg, keep = beam_cfg(sctc, beam=256, A=256, T=0)
    assert ws(cfg) > 0
    # LM tables are checked before any upload
    h = ctypes.c_void_p()
    k = np.zeros(16, np.uint64)
    p = np.zeros(16, np.float32)
    assert L.sctc_lm_create(k.ctypes.data, p.ctypes.data, p.ctypes.data, 15, 3, 1, ctypes.byref(h)) == -1
    assert L.sctc_lm_create(k.ctypes.data, p.ctypes.data, p.ctypes.data, 16, 9, 1, ctypes.byref(h)) == -1
    assert L.sctc_lm_create(k.ctypes.data, p.ctypes.data, p.ctypes.data, 16, 3, 0, ctypes.byref(h)) == -1
    assert L.sctc_lm_destroy(None) == 0


def test_python_argument_errors_need_no_gpu(sctc):
    import ctc_fast
    from new_decoder import decoder
    lp = [np.log(np.full((5, 4), 0.2))]
    for kw in (dict(beam=0), dict(beam=257), dict(nbest=2, beam=1)):
        with pytest.raises(ValueError):
            ctc_fast.decode_beam_batch(lp, **kw)
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch([np.zeros((300, 4))])
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch([np.zeros((5, 4)), np.zeros((6, 4))])
    with pytest.raises(ValueError):
        ctc_fast.decode_beam_batch(lp, lm="not an lm")
    d = decoder.BeamLMDecoder()
    d.load_chars(os.path.join(GOLDEN, "chars.txt"))
    with pytest.raises(ValueError):
        d.decode(np.ascontiguousarray(np.zeros((5, 4))))       # the memoryview wants Fortran order
    with pytest.raises(ValueError):
        d.decode(np.asfortranarray(np.zeros((5, 4), np.float32)))
    with pytest.raises(ValueError):
        d.decode(np.asfortranarray(np.zeros((5, 4))))           # no LM loaded
    assert d.int_char_map[1] == "[space]" and d.char_int_map["a"] == 2
    a = decoder.ArgmaxDecoder()
    with pytest.raises(ValueError):
        a.decode(np.zeros(5))
