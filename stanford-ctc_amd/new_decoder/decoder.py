"""Drop-in for the reference's Cython module ``ctc_fast/new_decoder/decoder.pyx``:
the same classes and calls, decoding on the MI355X through libsctc_hip.so.

    DecoderBase.load_chars(charmap_file)                            decoder.pyx:44-59
    ArgmaxDecoder.decode(probs) -> (hyp, score)                     decoder.pyx:79-100
    BeamLMDecoder.load_lm(lmfile)                                   decoder.pyx:108-114
    BeamLMDecoder.decode(probs, beam=40, alpha=1.0, beta=0.0)
        -> (hyp, score)                                             decoder.pyx:136-193

``probs`` is a float64 (A, T) Fortran-ordered array of natural-log probabilities, as the
``double[::1,:]`` memoryview accepts; anything else raises like the memoryview does.  The
LM is an ARPA file read by arpa_lm.py (kenlm is not needed), or -- a path ending in ``.npz`` -- the
neural character LM of nn_lm.py (with ``kind = "rnn"`` the recurrent one, §4.10).  ``decode_batch`` (not in
the reference) decodes a list of utterances in one launch.
"""
import numpy as np

import _sctc
import arpa_lm
import ctc_fast


def _check_probs(probs):
    if probs is None:
        raise TypeError("Argument 'probs' must not be None")
    if not isinstance(probs, np.ndarray):
        raise TypeError("Argument 'probs' has incorrect type (expected numpy.ndarray)")
    if probs.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % probs.ndim)
    if probs.dtype != np.float64:
        raise ValueError("Buffer dtype mismatch, expected 'double' but got '%s'" % probs.dtype)
    if not probs.flags.f_contiguous:
        raise ValueError("ndarray is not Fortran contiguous")


class DecoderBase(object):
    def __init__(self):
        self.char_int_map = None
        self.int_char_map = None

    def load_chars(self, charmap_file):
        """``token id`` per line -> char_int_map / int_char_map (decoder.pyx:44-59)"""
        with open(charmap_file) as fid:
            self.char_int_map = dict(tuple(l.strip().split()) for l in fid.readlines())
        self.int_char_map = {}
        for k, v in list(self.char_int_map.items()):
            self.char_int_map[k] = int(v)
            self.int_char_map[int(v)] = k
        return True

    def decode(self, probs):
        return None

    def _string(self, ids):
        return "".join(self.int_char_map[int(i)] for i in ids)


class ArgmaxDecoder(DecoderBase):
    """Per-frame argmax (first maximum wins), collapse repeats, drop blanks; the score is the
    sum of the argmax log-probabilities.  Unlike ctc_fast.decode_best_path it keeps ids
    1, 2 and 8 (decoder.pyx:79-100)."""

    def decode(self, probs):
        _check_probs(probs)
        torch = _sctc.require_gpu()
        A, T = probs.shape
        dev = torch.from_numpy(probs.T).cuda()
        best = torch.empty(max(T, 1), dtype=torch.int32, device=dev.device)
        if T:
            rc = _sctc.lib().sctc_argmax_rows(dev.data_ptr(), _sctc.F64, best.data_ptr(), T, A, A,
                                              _sctc.current_stream_ptr())
            _sctc.check(rc, "ArgmaxDecoder.decode")
        maxInd = best.cpu().numpy()[:T]
        hyp = []
        hyp_score = 0.0
        pmInd = -1
        for t in range(T):
            hyp_score = hyp_score + probs[maxInd[t], t]
            if maxInd[t] != pmInd:
                pmInd = maxInd[t]
                if pmInd > 0:
                    hyp.append(self.int_char_map[int(pmInd)])
        return "".join(hyp), hyp_score

    def decode_batch(self, probs_list):
        """[(hyp, score)] of a list of (A, T) arrays, one launch (``ctc_fast.decode_best_path_batch`` with only
        the blank dropped); the score is summed in float64 on the device, in the kernel's order"""
        for p in probs_list:
            if not isinstance(p, np.ndarray) or p.ndim != 2:
                raise ValueError("decode_batch: (A, T) arrays expected")
        ids, _, scores = ctc_fast.decode_best_path_batch(probs_list, blank=0, drop=(), scores=True)
        return [(self._string(h), float(s)) for h, s in zip(ids, scores)]


class BeamLMDecoder(DecoderBase):
    """Prefix beam search with a character LM (decoder.pyx:103-193), DESIGN.md §4.5."""

    def __init__(self):
        DecoderBase.__init__(self)
        self.lm = None
        self._dev = {}

    def load_lm(self, lmfile):
        if str(lmfile).endswith(".npz"):
            import nn_lm
            self.lm = nn_lm.load(lmfile)        # the window model or, kind = "rnn", the recurrent one
        else:
            self.lm = arpa_lm.ArpaLM(lmfile)
        self._dev = {}
        return True

    def _device_lm(self, A):
        if self.lm is None:
            raise ValueError("BeamLMDecoder: load_lm first")
        if self.int_char_map is None:
            raise ValueError("BeamLMDecoder: load_chars first")
        if A not in self._dev:
            import nn_lm
            cls = ctc_fast.DecodeLM if isinstance(self.lm, arpa_lm.ArpaLM) else \
                ctc_fast.DecodeRNNLM if isinstance(self.lm, nn_lm.RNNCharLM) else ctc_fast.DecodeNNLM
            self._dev[A] = cls(self.lm, self.int_char_map, A)
        return self._dev[A]

    def decode(self, probs, beam=40, alpha=1.0, beta=0.0):
        _check_probs(probs)
        (hyp, score), = self.decode_batch([probs], beam, alpha, beta)
        return hyp, score

    def _rescore_lm(self, lm, A):
        """the device handle of a second-pass LM: a ctc_fast.Decode*LM as it is, a model or the path of one uploaded
        once per alphabet"""
        if isinstance(lm, (ctc_fast.DecodeLM, ctc_fast.DecodeNNLM, ctc_fast.DecodeRNNLM)):
            return lm
        if self.int_char_map is None:
            raise ValueError("BeamLMDecoder: load_chars first")
        key = ("rescore", lm if isinstance(lm, str) else id(lm), A)
        if key not in self._dev:
            import nn_lm
            model = lm
            if isinstance(lm, str):
                model = nn_lm.load(lm) if lm.endswith(".npz") else arpa_lm.ArpaLM(lm)
            cls = ctc_fast.DecodeLM if isinstance(model, arpa_lm.ArpaLM) else \
                ctc_fast.DecodeRNNLM if isinstance(model, nn_lm.RNNCharLM) else ctc_fast.DecodeNNLM
            self._dev[key] = (cls(model, self.int_char_map, A), model)      # the model stays alive with its id
        return self._dev[key][0]

    def decode_batch(self, probs_list, beam=40, alpha=1.0, beta=0.0, nbest=1, rescore_lm=None, rescore_alpha=None,
                     rescore_beta=None, rescore_nbest=None, rescore_word_lm=None, rescore_word_alpha=1.0,
                     rescore_word_beta=0.0):
        """[(hyp, score)] for a list of (A, T) log-probability arrays, one launch; with nbest > 1 a list
        of nbest (hyp, score) per utterance, best first (ranks beyond the beam: '', -inf).

        ``rescore_lm`` (a ctc_fast.Decode*LM, a model, or the path of an ARPA / .npz file): a second pass
        (``ctc_fast.rescore_nbest``) re-ranks the leading ``rescore_nbest`` hypotheses of every
        utterance (default: all ``nbest``) by log P_ctc + rescore_alpha * log10 P_LM + rescore_beta * length under that
        LM (the weights default to the first pass's) and returns them in the new order with the new scores; the
        ranks it leaves alone follow with their first-pass scores.  ``self.rescore_changed`` then says, per
        utterance, whether the 1-best changed.

        ``rescore_word_lm`` (a ctc_fast.DecodeLexicon), alone or with ``rescore_lm``: the second pass adds
        rescore_word_alpha * (natural-log word-LM score) + rescore_word_beta * words.  Alone, the
        character-LM term of the second pass is left out; its length bonus rescore_beta * length (default: the first
        pass's ``beta``) stays -- pass ``rescore_beta=0.0`` for log P_ctc and the word term only."""
        if int(beam) < 0:
            raise OverflowError("can't convert negative value to unsigned int")
        for p in probs_list:
            if not isinstance(p, np.ndarray) or p.ndim != 2:
                raise ValueError("decode_batch: (A, T) arrays expected")
        A = probs_list[0].shape[0]
        ids, scores = ctc_fast.decode_beam_batch(probs_list, beam=beam, alpha=alpha, beta=beta,
                                                 lm=self._device_lm(A), nbest=nbest)
        if rescore_lm is not None or rescore_word_lm is not None:
            rows = ids if nbest > 1 else [[h] for h in ids]
            first = np.array(scores, dtype=np.float64).reshape(len(rows), nbest)
            seen = first.copy()
            if rescore_nbest is not None:
                if not 1 <= int(rescore_nbest) <= nbest:
                    raise ValueError("decode_batch: rescore_nbest outside 1..nbest")
                seen[:, int(rescore_nbest):] = -np.inf
            order, res = ctc_fast.rescore_nbest(probs_list, rows,
                                                lm=self._rescore_lm(rescore_lm, A) if rescore_lm is not None else None,
                                                alpha=alpha if rescore_alpha is None else rescore_alpha,
                                                beta=beta if rescore_beta is None else rescore_beta, scores=seen,
                                                word_lm=rescore_word_lm, word_alpha=rescore_word_alpha,
                                                word_beta=rescore_word_beta)
            self.rescore_changed = [int(o[0]) != 0 for o in order]
            out = [[(self._string(row[k]), float(res[b, k]) if seen[b, k] > -np.inf else float(first[b, k])) for k in o]
                   for b, (row, o) in enumerate(zip(rows, order))]
            return out if nbest > 1 else [r[0] for r in out]
        if nbest > 1:
            return [[(self._string(h), float(s)) for h, s in zip(row, srow)] for row, srow in zip(ids, scores)]
        return [(self._string(h), float(s)) for h, s in zip(ids, scores)]

    def score(self, probs, label_ids, alpha=1.0, beta=0.0):
        """The score of the symbol-id row ``label_ids`` under the objective that :meth:`decode`
        maximises (``ctc_fast.score_sentences``): the refScore that
        decoder_utils.py:68-70 left open.  -inf when the row cannot be aligned to ``probs``."""
        _check_probs(probs)
        return float(ctc_fast.score_sentences([probs], [label_ids], lm=self._device_lm(probs.shape[0]),
                                              alpha=alpha, beta=beta)[0])

    def align(self, probs, label_ids):
        """The best alignment of ``label_ids`` to ``probs`` (``ctc_fast.align_batch``): (frame_label
        int32 [T], spans int32 [U, 2], viterbi score, status)."""
        _check_probs(probs)
        fl, spans, vit, _, status = ctc_fast.align_batch([probs], [label_ids])
        return fl[0], spans[0], float(vit[0]), int(status[0])
