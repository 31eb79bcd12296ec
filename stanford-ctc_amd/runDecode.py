"""Decode a likelihood shard (the flow of the reference's ctc_fast/new_decoder/test_simple.py
and runDecode.py:41-77): read ``loglikelihoods_N.pk`` (writeLikelihoods.py), ``chars.txt``,
the alignment file and an ARPA character LM; decode every utterance with the prefix beam
search on the GPU, in batches; write one hypothesis per line and report the character error
rate against the alignments: one batched edit-distance launch per decode batch
(ctc_fast.edit_distance_batch).

    python runDecode.py --likelihoods loglikelihoods_1.pk --chars chars.txt --alis alis1.txt \\
        --lm text_char.2g.arpa --out hyps.txt [--beam 40 --alpha 1.0 --beta 0.0 --batch 256]

``--method bg`` decodes to words instead (the reference's ``decoder_utils.decode(..., method='bg')``,
ctc_fast/decoder/bg_decoder.pyx): a word list constrains the spellings, an ARPA word-bigram LM
scores every finished word, hypotheses are written as words, and the word error rate is reported
next to the character error rate (reference words: the alignment split at the space symbol).

    python runDecode.py --method bg --likelihoods loglikelihoods_1.pk --chars chars.txt --alis alis1.txt \\
        --words wordlist --word-lm text_word.2g.arpa --out hyps.txt [--specials [noise] [laughter]]
        [--word-lm-order 3]

``--errors FILE`` writes ``key dist ins dels subs corr`` for every scored utterance (characters
against the alignment, the naming of editDistance.py) and adds a line of totals to the summary;
``--nbest-oracle K`` (character method) decodes K hypotheses per utterance and prints the CER of
the best of them next to the 1-best CER.

``--ref-scores FILE`` writes ``key hypscore refscore`` per utterance with a
transcript: the transcript scored under the objective the search maximises
(ctc_fast.score_sentences; the refScore that the reference's decoder_utils.py:68-70
left open), and adds a line that counts the search errors (refscore > hypscore) and the transcripts
that cannot be aligned.  ``--ctm FILE [--frame-shift 0.01]`` writes the 1-best hypotheses as a CTM
(swbd-utils/convert_to_ctm.py:21-37) with the time of every word taken from the forced alignment of
the hypothesis (ctc_fast.align_batch): words are the runs of labels between ``--space`` symbols.

``--rescore-lm FILE --rescore-nbest K [--rescore-alpha --rescore-beta]`` (character method, K <= beam) adds a
second pass (ctc_fast.rescore_nbest): the K best hypotheses of the search are re-ranked under the
LM of FILE (ARPA, or the .npz of a neural LM) with the full CTC sum; the hypothesis file and the CER are those of the
re-ranked 1-best, and the summary says how many utterances changed their 1-best.
``--rescore-word-lm ARPA --rescore-words WORDLIST [--rescore-word-lm-order N --rescore-word-alpha --rescore-word-beta]``,
alone or next to ``--rescore-lm``, puts a word LM into that second pass: the character LM finds the
hypotheses, the word LM orders them; a word outside WORDLIST scores as ``<UNK>``.  The word LM's score is in natural
log, so its weight means what ``--alpha`` means for ``--method bg``.

With ``--method bg``, ``--ref-scores FILE`` scores the transcript under the word search's objective: log P_ctc +
alpha * (word-LM terms of the words a space follows) + beta * (those words).
"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ctc_fast  # noqa: E402
import editDistance  # noqa: E402
from new_decoder import decoder  # noqa: E402
from decoder import decoder_utils  # noqa: E402


def edit_distance(ref, hyp):
    """Levenshtein distance between two sequences"""
    prev = list(range(len(hyp) + 1))
    for i in range(1, len(ref) + 1):
        cur = [i] + [0] * len(hyp)
        for j in range(1, len(hyp) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ref[i - 1] != hyp[j - 1]))
        prev = cur
    return prev[-1]


def score_pairs(refs, hyps):
    """int32 [P, 5] (dist, ins, dels, subs, corr; editDistance.py naming) of token sequences, one launch"""
    ids = editDistance._ids(list(refs) + list(hyps))
    return ctc_fast.edit_distance_batch(ids[:len(refs)], ids[len(refs):])


class ErrorLog(object):
    """--errors FILE: one line per scored utterance and the totals; a context manager, so the file is closed
    when decoding raises"""

    def __init__(self, path):
        self.f = open(path, "w") if path else None
        self.total = np.zeros(5, dtype=np.int64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.f:
            self.f.close()

    def add(self, key, stats):
        self.total += stats
        if self.f:
            self.f.write("%s %d %d %d %d %d\n" % ((key,) + tuple(int(v) for v in stats)))

    def summary(self):
        if self.f:
            print("errors %d: ins %d, dels %d, subs %d, corr %d" % tuple(int(v) for v in self.total))


class RefScoreLog(object):
    """--ref-scores FILE: ``key hypscore refscore`` per utterance with a transcript; counts the search errors
    (the transcript scores higher than the hypothesis that the search returned) and the transcripts that
    cannot be aligned"""

    def __init__(self, path):
        self.f = open(path, "w") if path else None
        self.n = self.search_errors = self.unaligned = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.f:
            self.f.close()

    def add(self, key, hyp_score, ref_score):
        self.n += 1
        self.search_errors += int(ref_score > hyp_score)
        self.unaligned += int(ref_score == -np.inf)
        self.f.write("%s %.6f %.6f\n" % (key, hyp_score, ref_score))

    def summary(self):
        if self.f:
            print("ref scores of %d transcripts: %d search errors (refscore > hypscore), %d without an alignment"
                  % (self.n, self.search_errors, self.unaligned))


CTM_FORM = "%s %s %0.2f %0.2f %s\n"     # convert_to_ctm.py:21


def parse_ctm_key(key):
    """(file id, channel, segment offset in seconds) of an utterance key, convert_to_ctm.py:27-34: the third
    ``_`` field is ``start-end`` in centiseconds, the file id the first seven characters, the channel A where
    the key holds ``-a_``, else B.  A key that does not parse that way: (key, 'A', 0.0)."""
    try:
        times = key.split("_")[2]
        start, _end = [int(x) / 100.0 for x in times.split("-")]
    except (IndexError, ValueError):
        return key, "A", 0.0
    return key[0:7], "A" if "-a_" in key else "B", start


def ctm_words(ids, spans, space_id, int_char_map):
    """[(word, first frame, last frame)]: the maximal runs of labels between space symbols, with the first
    frame of the first label and the last frame of the last one (inclusive); none for a row without an alignment"""
    out, run = [], []
    if len(ids) and np.asarray(spans).min() < 0:    # no alignment (status != 0): no times to give
        return out
    for u, c in enumerate(list(ids) + [space_id]):
        if c == space_id or u == len(ids):
            if run:
                out.append(("".join(int_char_map[int(ids[i])] for i in run), int(spans[run[0]][0]), int(spans[run[-1]][1])))
            run = []
        else:
            run.append(u)
    return out


def ctm_lines(key, words, frame_shift):
    """the CTM lines of one utterance: start = segment offset + first frame * shift, duration = (last frame
    + 1 - first frame) * shift"""
    file_id, channel, offset = parse_ctm_key(key)
    return [CTM_FORM % (file_id, channel, offset + first * frame_shift, (last + 1 - first) * frame_shift, w)
            for w, first, last in words]


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


def decode_bg(a, ll):
    """--method bg: (CER, WER) of the lexicon-constrained search with a word bigram, or a word n-gram of
    --word-lm-order"""
    chars = decoder_utils.load_chars(a.chars)
    alis = load_alis(a.alis, a.chars)
    lex = ctc_fast.DecodeLexicon(a.words, chars, a.word_lm, a.space, specials=a.specials, order=a.word_lm_order)
    keys = sorted(ll)
    errs = n_ref = werrs = n_words = 0
    with open(a.out, "w") as out, ErrorLog(a.errors) as log, RefScoreLog(a.ref_scores) as ref_log:
        for g in range(0, len(keys), a.batch):
            ks = keys[g:g + a.batch]
            hyps, scores = ctc_fast.decode_lexicon_beam_batch([np.asarray(ll[k]) for k in ks], lexicon=lex,
                                                              beam=a.beam, alpha=a.alpha, beta=a.beta)
            if ref_log.f:       # the transcripts under the search's objective: words finished, no character LM
                idx = [i for i, k in enumerate(ks) if k in alis]
                if idx:
                    ref_ids = [[chars.get(t, -1) for t in alis[ks[i]]] for i in idx]
                    ref_scores = ctc_fast.score_sentences([np.asarray(ll[ks[i]]) for i in idx], ref_ids, word_lm=lex,
                                                          word_alpha=a.alpha, word_beta=a.beta, word_final=False)
                    for i, rs in zip(idx, ref_scores):
                        ref_log.add(ks[i], scores[i], rs)
            scored, refs, cand = [], [], []
            for k, ids, score in zip(ks, hyps, scores):
                toks = decoder_utils.int_to_char(ids, chars)
                words = decoder_utils.collapse_seq(toks, a.space)
                out.write("%s %.6f %s\n" % (k, score, words))
                if k in alis:
                    scored.append(k)
                    refs += [alis[k], decoder_utils.collapse_seq(alis[k], a.space).split()]
                    cand += [toks, words.split()]
            # characters and words of the whole decode batch in one launch: pairs 2i and 2i + 1
            stats = score_pairs(refs, cand)
            for i, k in enumerate(scored):
                errs += int(stats[2 * i, 0])
                n_ref += len(refs[2 * i])
                werrs += int(stats[2 * i + 1, 0])
                n_words += len(refs[2 * i + 1])
                log.add(k, stats[2 * i])
    cer = errs / float(max(n_ref, 1))
    wer = werrs / float(max(n_words, 1))
    print("decoded %d utterances, CER %.4f (%d / %d), WER %.4f (%d / %d)"
          % (len(keys), cer, errs, n_ref, wer, werrs, n_words))
    log.summary()
    ref_log.summary()
    return cer, wer


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--likelihoods", required=True)
    ap.add_argument("--chars", required=True)
    ap.add_argument("--alis", required=True)
    ap.add_argument("--lm", help="ARPA character LM (the default method)")
    ap.add_argument("--method", choices=("char", "bg"), default="char",
                    help="char: character LM (default); bg: word list and word-bigram LM")
    ap.add_argument("--words", help="word list, one per line (--method bg)")
    ap.add_argument("--word-lm", help="ARPA word LM (--method bg)")
    ap.add_argument("--word-lm-order", type=int, default=2,
                    help="order 2..5 at which --word-lm is read: 2 is the reference's word bigram, 3..5 use the "
                         "file's higher sections too (default 2)")
    ap.add_argument("--specials", nargs="*", default=[], help="tokens of chars.txt that are whole words")
    ap.add_argument("--space", default="[space]", help="the word separator token of chars.txt")
    ap.add_argument("--out", required=True)
    ap.add_argument("--beam", type=int, default=40)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--errors", help="write `key dist ins dels subs corr` per scored utterance to this file")
    ap.add_argument("--nbest-oracle", type=int, default=0, metavar="K",
                    help="also report the CER of the best of K hypotheses per utterance (character method, K <= beam)")
    ap.add_argument("--ref-scores", metavar="FILE",
                    help="write `key hypscore refscore` per utterance with a transcript: the transcript scored under "
                         "the search's own objective (either method)")
    ap.add_argument("--ctm", metavar="FILE",
                    help="write a CTM with the time of every word of the 1-best hypotheses, from their forced "
                         "alignment (character method)")
    ap.add_argument("--frame-shift", type=float, default=0.01, help="seconds per frame (--ctm)")
    ap.add_argument("--rescore-lm", metavar="FILE",
                    help="second pass: re-rank the --rescore-nbest best hypotheses under this LM (character method)")
    ap.add_argument("--rescore-nbest", type=int, default=0, metavar="K", help="hypotheses re-ranked per utterance, K <= beam")
    ap.add_argument("--rescore-alpha", type=float, default=None, help="LM weight of the second pass (default --alpha)")
    ap.add_argument("--rescore-beta", type=float, default=None, help="length bonus of the second pass (default --beta)")
    ap.add_argument("--rescore-word-lm", metavar="ARPA",
                    help="second pass: add a word LM's score over the words of the --rescore-nbest best hypotheses, "
                         "alone or with --rescore-lm; needs --rescore-words (character method)")
    ap.add_argument("--rescore-words", metavar="WORDLIST", help="word list of --rescore-word-lm, one per line")
    ap.add_argument("--rescore-word-lm-order", type=int, default=2, help="order 2..5 at which --rescore-word-lm is read")
    ap.add_argument("--rescore-word-alpha", type=float, default=1.0,
                    help="weight of the word LM's natural-log score in the second pass (default 1)")
    ap.add_argument("--rescore-word-beta", type=float, default=0.0, help="bonus per word of the second pass (default 0)")
    ap.add_argument("--wer", action="store_true",
                    help="also print the word error rate of the character method: the words interned on the device "
                         "(ctc_fast.word_errors_batch), so that distinct out-of-vocabulary words stay distinct")
    ap.add_argument("--mbr", choices=("char", "word"),
                    help="write the minimum Bayes risk hypothesis of the n-best list instead of the top-ranked one: least "
                         "expected edit distance in symbols or in words under the list's posteriors (ctc_fast.mbr_nbest); "
                         "the list is that of --rescore-nbest K with its second-pass scores, or the first pass's --mbr-nbest K")
    ap.add_argument("--mbr-scale", type=float, default=None, help="posterior scale of --mbr (default 1): w = exp(S * (s - s_max))")
    ap.add_argument("--mbr-nbest", type=int, default=0, metavar="K", help="hypotheses of the first pass under --mbr, K <= beam")
    ap.add_argument("--ctm-conf", action="store_true",
                    help="with --ctm and --mbr word: a sixth CTM column, the posterior mass of the hypotheses that agree with the word")
    a = ap.parse_args(argv)
    K = a.nbest_oracle
    if (a.mbr or a.mbr_nbest or a.mbr_scale is not None or a.ctm_conf) and a.method == "bg":
        ap.error("--mbr, --mbr-scale, --mbr-nbest and --ctm-conf are for the character method")
    if not a.mbr and (a.mbr_nbest or a.mbr_scale is not None):
        ap.error("--mbr-nbest and --mbr-scale need --mbr {char,word}")
    if a.mbr and bool(a.mbr_nbest) == bool(a.rescore_nbest):
        ap.error("--mbr needs the list of --rescore-nbest K or of --mbr-nbest K, one of the two")
    if a.mbr_nbest and not 1 <= a.mbr_nbest <= a.beam:
        ap.error("--mbr-nbest K needs 1 <= K <= beam")
    if a.mbr_scale is not None and not (np.isfinite(a.mbr_scale) and a.mbr_scale >= 0):
        ap.error("--mbr-scale must be a finite number >= 0")
    if a.ctm_conf and not (a.ctm and a.mbr == "word"):
        ap.error("--ctm-conf needs --ctm FILE and --mbr word")
    if a.wer and a.method == "bg":
        ap.error("--wer is for the character method (--method bg reports its WER already)")
    if K and a.method == "bg":
        ap.error("--nbest-oracle is for the character method")
    if a.ctm and a.method == "bg":
        ap.error("--ctm is for the character method")
    if K and not 1 <= K <= a.beam:
        ap.error("--nbest-oracle K needs 1 <= K <= beam")
    Kr = a.rescore_nbest
    if (a.rescore_lm or a.rescore_word_lm or Kr) and a.method == "bg":
        ap.error("--rescore-lm and --rescore-word-lm are for the character method")
    if bool(a.rescore_word_lm) != bool(a.rescore_words):
        ap.error("--rescore-word-lm ARPA needs --rescore-words WORDLIST, and the other way round")
    if bool(a.rescore_lm or a.rescore_word_lm) != bool(Kr) or (Kr and not 1 <= Kr <= a.beam):
        ap.error("--rescore-lm FILE / --rescore-word-lm ARPA need --rescore-nbest K with 1 <= K <= beam, and the other "
                 "way round")
    with open(a.likelihoods, "rb") as f:
        ll = pickle.load(f)
    if a.method == "bg":
        if not a.words or not a.word_lm:
            ap.error("--method bg needs --words and --word-lm")
        return decode_bg(a, ll)
    if not a.lm:
        ap.error("--lm is required")
    alis = load_alis(a.alis, a.chars)
    dec = decoder.BeamLMDecoder()
    dec.load_chars(a.chars)
    dec.load_lm(a.lm)
    word_lex = None
    if a.rescore_word_lm:
        word_lex = ctc_fast.DecodeLexicon(a.rescore_words, dec.char_int_map, a.rescore_word_lm, a.space,
                                          specials=a.specials, A=np.asarray(ll[sorted(ll)[0]]).shape[0] if ll else None,
                                          order=a.rescore_word_lm_order)
    keys = sorted(ll)
    errs = n_ref = oracle_errs = n_changed = 0
    w_errs = w_ref = 0
    space_id = dec.char_int_map.get(a.space)
    if (a.wer or a.mbr == "word") and space_id is None:
        ap.error("--wer and --mbr word need the word separator %s in --chars" % a.space)
    Km = Kr or a.mbr_nbest
    n_mbr_changed = 0
    n_sym = max(dec.char_int_map.values()) + 2      # --wer, --mbr: a token the map does not know is a symbol of its own
    if (a.wer or a.mbr) and n_sym > 256:
        ap.error("--wer and --mbr take character maps of at most 254 symbols, --chars has ids up to %d" % (n_sym - 2))
    with open(a.out, "w") as out, ErrorLog(a.errors) as log, RefScoreLog(a.ref_scores) as ref_log, \
            open(a.ctm or os.devnull, "w") as ctm:
        for g in range(0, len(keys), a.batch):
            ks = keys[g:g + a.batch]
            probs = [np.asfortranarray(ll[k], dtype=np.float64) for k in ks]
            if Kr:
                res = dec.decode_batch(probs, a.beam, a.alpha, a.beta, nbest=max(K, Kr), rescore_lm=a.rescore_lm,
                                       rescore_alpha=a.rescore_alpha, rescore_beta=a.rescore_beta, rescore_nbest=Kr,
                                       rescore_word_lm=word_lex, rescore_word_alpha=a.rescore_word_alpha,
                                       rescore_word_beta=a.rescore_word_beta)
                n_changed += sum(dec.rescore_changed)
            else:
                res = dec.decode_batch(probs, a.beam, a.alpha, a.beta, nbest=max(K, a.mbr_nbest, 1))
            if max(K, Kr, a.mbr_nbest) <= 1:
                res = [[r] for r in res]
            conf = None
            if a.mbr:           # the first Km ranks of every list, in the order the pass left them: ties go to the earlier
                cand_ids = [[[dec.char_int_map.get(t, n_sym - 1) for t in tokens(h, dec.char_int_map)] for h, _ in row[:Km]]
                            for row in res]
                m = ctc_fast.mbr_nbest(cand_ids, [[s for _, s in row[:Km]] for row in res], unit=a.mbr,
                                       scale=1.0 if a.mbr_scale is None else a.mbr_scale, space=space_id, A=n_sym,
                                       confidences=a.ctm_conf)
                conf = m.get("confidence")
                pick = [max(int(b), 0) for b in m["best"]]
                n_mbr_changed += sum(b != 0 for b in pick)
                res = [[row[b]] + row[:b] + row[b + 1:] for row, b in zip(res, pick)]
            if ref_log.f:       # the transcripts of the batch under the search's objective, one call
                idx = [i for i, k in enumerate(ks) if k in alis]
                ref_ids = [[dec.char_int_map.get(t, -1) for t in alis[ks[i]]] for i in idx]
                if idx:
                    ref_scores = ctc_fast.score_sentences([probs[i] for i in idx], ref_ids, alpha=a.alpha, beta=a.beta,
                                                          lm=dec._device_lm(probs[0].shape[0]))
                    for i, rs in zip(idx, ref_scores):
                        ref_log.add(ks[i], res[i][0][1], rs)
            if a.ctm:           # every 1-best hypothesis aligned to its own utterance, one call
                hyp_ids = [[dec.char_int_map[t] for t in tokens(row[0][0], dec.char_int_map)] for row in res]
                _, spans, _, _, _ = ctc_fast.align_batch(probs, hyp_ids)
                for i, (k, ids, sp) in enumerate(zip(ks, hyp_ids, spans)):
                    lines = ctm_lines(k, ctm_words(ids, sp, space_id, dec.int_char_map), a.frame_shift)
                    if a.ctm_conf:      # an utterance without an alignment has no lines
                        lines = ["%s %.4f\n" % (l[:-1], c) for l, c in zip(lines, conf[i])]
                    ctm.writelines(lines)
            scored, refs, cand, lists = [], [], [], []
            for k, row in zip(ks, res):
                out.write("%s %.6f %s\n" % (k, row[0][1], row[0][0]))
                if k in alis:
                    scored.append(k)
                    refs.append(alis[k])
                    cand.append(tokens(row[0][0], dec.char_int_map))
                    # ranks beyond the beam (score -inf) are no hypotheses; rank 0 always is
                    lists.append([cand[-1]] + [tokens(h, dec.char_int_map) for h, s in row[1:] if s > -np.inf])
            stats = score_pairs(refs, cand)
            for k, ref, st in zip(scored, refs, stats):
                errs += int(st[0])
                n_ref += len(ref)
                log.add(k, st)
            if a.wer and refs:
                rows = [[dec.char_int_map.get(t, n_sym - 1) for t in r] for r in refs + cand]
                st = ctc_fast.word_errors_batch(rows[:len(refs)], rows[len(refs):], space_id, A=n_sym)
                w_errs += int(st[:, 0].sum())
                w_ref += int((st[:, 1] + st[:, 3] + st[:, 4]).sum())      # a = ref: every word of it is UP, SUB or MATCH
            if K:
                table = {}
                ids = [[table.setdefault(t, len(table)) for t in r] for r in refs]
                nb = [[[table.setdefault(t, len(table)) for t in h] for h in row] for row in lists]
                oracle_errs += int(ctc_fast.nbest_oracle(ids, nb)[1].sum()) if ids else 0
    cer = errs / float(max(n_ref, 1))
    print("decoded %d utterances, CER %.4f (%d / %d)" % (len(keys), cer, errs, n_ref))
    if a.wer:
        print("WER %.4f (%d / %d words)" % (w_errs / float(max(w_ref, 1)), w_errs, w_ref))
    log.summary()
    ref_log.summary()
    if Kr:
        print("rescored: %d of %d utterances changed their 1-best" % (n_changed, len(keys)))
    if a.mbr:
        print("mbr (%s): %d of %d utterances changed their 1-best" % (a.mbr, n_mbr_changed, len(keys)))
    if K:
        print("oracle CER of %d-best %.4f (%d / %d), 1-best CER %.4f (%d / %d)"
              % (K, oracle_errs / float(max(n_ref, 1)), oracle_errs, n_ref, cer, errs, n_ref))
    return cer


if __name__ == "__main__":
    main()
