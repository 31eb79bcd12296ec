"""Drop-in for the reference's ``decoder/bg_decoder.pyx``:

    decode_bg_lm(probs, prefixTree, lm, beam=40, alpha=1.0, beta=0.0) -> (symbol ids, score)

``probs`` is a float64 (A, T) Fortran-ordered array of natural-log probabilities, as the
``double[::1,:] probs not None`` signature accepts; anything else raises like the memoryview
does.  The search runs on the GPU (csrc/ctc_beam.hip); the tree and the LM are
uploaded once per (tree, alphabet size) and kept on the tree object.  ``lm`` is a ``decoder.lm.LM``
(the reference's word bigram) or a ``decoder.ngram_lm.NgramLM`` of order 2..5 (§4.6b), for which the
LM term of a finished word is ``alpha * P(word | the last order-1 words)``.  ``decode_bg_lm_batch``
(not in the reference) decodes a list of utterances in one launch."""
import numpy as np

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


def _device_lexicon(prefixTree, lm, A):
    cache = prefixTree.__dict__.setdefault("_device_lexica", {})
    key = (id(lm), int(A))
    if key not in cache:
        cache[key] = ctc_fast.DecodeLexicon.from_tree(prefixTree, lm, A)
    return cache[key]


def decode_bg_lm_batch(probs_list, prefixTree, lm, beam=40, alpha=1.0, beta=0.0):
    """[(symbol ids, score)] for a list of (A, T) log-probability arrays, one launch"""
    if int(beam) < 0:
        raise OverflowError("can't convert negative value to unsigned int")
    for p in probs_list:
        if not isinstance(p, np.ndarray) or p.ndim != 2:
            raise ValueError("decode_bg_lm_batch: (A, T) arrays expected")
    A = probs_list[0].shape[0]
    ids, scores = ctc_fast.decode_lexicon_beam_batch(probs_list, lexicon=_device_lexicon(prefixTree, lm, A),
                                                     beam=beam, alpha=alpha, beta=beta)
    return [([int(i) for i in h], float(s)) for h, s in zip(ids, scores)]


def decode_bg_lm(probs, prefixTree, lm, beam=40, alpha=1.0, beta=0.0):
    _check_probs(probs)
    (hyp, score), = decode_bg_lm_batch([probs], prefixTree, lm, beam, alpha, beta)
    return hyp, score
