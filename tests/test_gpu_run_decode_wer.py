"""runDecode.py --wer, --mbr and --ctm-conf: the character method's word error rate from words interned
on the device equals a host count over the split token lists, and the flag changes nothing else (the same output file,
the same other lines); the MBR hypothesis and the CTM confidences are those of tests/mbr_model.py."""
import os

import numpy as np
import pytest

from tests.test_gpu_rescore import GOLDEN, shard_likelihoods  # noqa: F401  (the fixture: the golden shard through a small BRNN)

pytestmark = pytest.mark.gpu


def split_words(toks, space):
    words, cur = [], []
    for t in toks:
        if t == space:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(t)
    if cur:
        words.append(tuple(cur))
    return words


def test_wer_line_equals_a_host_count(shard_likelihoods, tmp_path, capsys):  # noqa: F811
    import editDistance
    import runDecode
    chars = os.path.join(GOLDEN, "chars.txt")
    alis_file = os.path.join(GOLDEN, "shard", "alis1.txt")
    common = ["--likelihoods", shard_likelihoods, "--chars", chars, "--alis", alis_file,
              "--lm", os.path.join(GOLDEN, "lm_char_2g.arpa"), "--beam", "8", "--alpha", "0.5", "--beta", "0.3", "--batch", "3"]
    plain, with_wer = tmp_path / "plain.txt", tmp_path / "wer.txt"
    runDecode.main(common + ["--out", str(plain)])
    said_plain = capsys.readouterr().out.splitlines()
    assert not [l for l in said_plain if l.startswith("WER ")]
    runDecode.main(common + ["--out", str(with_wer), "--wer"])
    said = capsys.readouterr().out.splitlines()
    assert plain.read_bytes() == with_wer.read_bytes()
    line = [l for l in said if l.startswith("WER ")]
    assert len(line) == 1 and [l for l in said if not l.startswith("WER ")] == said_plain
    # the host count: the tokens of the reference and of the written hypothesis, cut at the space token
    from new_decoder import decoder
    d = decoder.BeamLMDecoder()
    d.load_chars(chars)
    alis = runDecode.load_alis(alis_file, chars)
    errs = n_words = 0
    for l in plain.read_text().splitlines():
        key, _, hyp = l.split(" ", 2)
        if key not in alis:
            continue
        ref_w = split_words(alis[key], "[space]")
        hyp_w = split_words(runDecode.tokens(hyp, d.char_int_map), "[space]")
        errs += int(editDistance.edit_distance(ref_w, hyp_w)[0])
        n_words += len(ref_w)
    assert n_words > 0
    assert line[0] == "WER %.4f (%d / %d words)" % (errs / float(n_words), errs, n_words)
    with pytest.raises(SystemExit):
        runDecode.main(["--likelihoods", shard_likelihoods, "--chars", chars, "--alis", alis_file, "--method", "bg",
                        "--words", chars, "--word-lm", chars, "--out", str(with_wer), "--wer"])


def test_mbr_word_and_ctm_confidences(shard_likelihoods, tmp_path, capsys):  # noqa: F811
    """--mbr word --mbr-nbest 4 --ctm-conf: the written hypothesis is the model's choice among the first pass's 4-best,
    and the CTM has six columns whose last is the model's confidence of the word"""
    import pickle
    import runDecode
    from new_decoder import decoder
    from tests import mbr_model as M
    chars = os.path.join(GOLDEN, "chars.txt")
    alis_file = os.path.join(GOLDEN, "shard", "alis1.txt")
    lm2 = os.path.join(GOLDEN, "lm_char_2g.arpa")
    common = ["--likelihoods", shard_likelihoods, "--chars", chars, "--alis", alis_file, "--lm", lm2, "--beam", "8",
              "--alpha", "0.5", "--beta", "0.3", "--batch", "3"]
    out, ctm, plain_ctm = tmp_path / "mbr.txt", tmp_path / "mbr.ctm", tmp_path / "plain.ctm"
    runDecode.main(common + ["--out", str(out), "--mbr", "word", "--mbr-nbest", "4", "--mbr-scale", "0.5", "--ctm", str(ctm),
                             "--ctm-conf"])
    said = capsys.readouterr().out
    assert len([l for l in said.splitlines() if l.startswith("mbr (word): ")]) == 1
    with open(shard_likelihoods, "rb") as f:
        pk = pickle.load(f)
    d = decoder.BeamLMDecoder()
    d.load_chars(chars)
    d.load_lm(lm2)
    space = d.char_int_map["[space]"]
    n_sym = max(d.char_int_map.values()) + 2
    keys = sorted(pk)
    got = out.read_text().splitlines()
    want_conf = []
    for g in range(0, len(keys), 3):
        ks = keys[g:g + 3]
        probs = [np.asfortranarray(pk[k], dtype=np.float64) for k in ks]
        rows = d.decode_batch(probs, 8, 0.5, 0.3, nbest=4)
        ids = [[[d.char_int_map[t] for t in runDecode.tokens(h, d.char_int_map)] for h, _ in row] for row in rows]
        m = M.mbr(ids, [[s for _, s in row] for row in rows], unit="word", scale=0.5, space=space, A=n_sym, confidences=True)
        for k, row, b, c in zip(ks, rows, m["best"], m["confidence"]):
            assert got[keys.index(k)] == "%s %.6f %s" % (k, row[b][1], row[b][0])
            want_conf += ["%.4f" % v for v in c]
    lines = ctm.read_text().splitlines()
    assert lines and all(len(l.split()) == 6 for l in lines)
    assert [l.split()[5] for l in lines] == want_conf
    assert all(0.0 <= float(v) <= 1.0 for v in want_conf)
    # the first five columns are those of the plain CTM of the same hypotheses; and a list of one changes nothing
    runDecode.main(common + ["--out", str(tmp_path / "one.txt"), "--mbr", "char", "--mbr-nbest", "1", "--ctm", str(plain_ctm)])
    capsys.readouterr()
    runDecode.main(common + ["--out", str(tmp_path / "first.txt")])
    assert (tmp_path / "one.txt").read_bytes() == (tmp_path / "first.txt").read_bytes()
    assert all(len(l.split()) == 5 for l in plain_ctm.read_text().splitlines())
    for bad in (["--mbr", "word"], ["--mbr-nbest", "4"], ["--mbr", "char", "--mbr-nbest", "4", "--ctm", str(ctm), "--ctm-conf"],
                ["--mbr", "word", "--mbr-nbest", "9"], ["--mbr", "word", "--mbr-nbest", "4", "--mbr-scale", "-1"]):
        with pytest.raises(SystemExit):
            runDecode.main(common + ["--out", str(out)] + bad)


def test_mbr_over_the_second_pass_list(shard_likelihoods, tmp_path, capsys):  # noqa: F811
    """--mbr char with --rescore-nbest 4: the list is the decoder's re-ranked one, with its second-pass scores and its
    order for ties; the written hypothesis is the model's choice on exactly that list"""
    import pickle
    import runDecode
    from new_decoder import decoder
    from tests import mbr_model as M
    chars = os.path.join(GOLDEN, "chars.txt")
    lm2 = os.path.join(GOLDEN, "lm_char_2g.arpa")
    rnn = os.path.join(GOLDEN, "lm_char_rnn.npz")
    common = ["--likelihoods", shard_likelihoods, "--chars", chars, "--alis", os.path.join(GOLDEN, "shard", "alis1.txt"),
              "--lm", lm2, "--beam", "8", "--alpha", "0.5", "--beta", "0.3", "--batch", "3"]
    second = ["--rescore-lm", rnn, "--rescore-nbest", "4", "--rescore-alpha", "1.5"]
    out = tmp_path / "mbr2.txt"
    runDecode.main(common + second + ["--out", str(out), "--mbr", "char", "--mbr-scale", "0.5"])
    said = capsys.readouterr().out.splitlines()
    assert len([l for l in said if l.startswith("rescored: ")]) == 1 and len([l for l in said if l.startswith("mbr (char): ")]) == 1
    with open(shard_likelihoods, "rb") as f:
        pk = pickle.load(f)
    d = decoder.BeamLMDecoder()
    d.load_chars(chars)
    d.load_lm(lm2)
    n_sym = max(d.char_int_map.values()) + 2
    keys = sorted(pk)
    got = out.read_text().splitlines()
    assert len(got) == len(keys)
    moved = 0
    for g in range(0, len(keys), 3):
        ks = keys[g:g + 3]
        probs = [np.asfortranarray(pk[k], dtype=np.float64) for k in ks]
        rows = d.decode_batch(probs, 8, 0.5, 0.3, nbest=4, rescore_lm=rnn, rescore_alpha=1.5)
        ids = [[[d.char_int_map[t] for t in runDecode.tokens(h, d.char_int_map)] for h, _ in row] for row in rows]
        m = M.mbr(ids, [[s for _, s in row] for row in rows], unit="char", scale=0.5, A=n_sym)
        for k, row, b in zip(ks, rows, m["best"]):
            assert got[keys.index(k)] == "%s %.6f %s" % (k, row[b][1], row[b][0])
            moved += int(b != 0)
    assert [l for l in said if l.startswith("mbr (char): ")][0] == "mbr (char): %d of %d utterances changed their 1-best" % (moved, len(keys))
    with pytest.raises(SystemExit):         # both lists at once
        runDecode.main(common + second + ["--out", str(out), "--mbr", "char", "--mbr-nbest", "4"])
