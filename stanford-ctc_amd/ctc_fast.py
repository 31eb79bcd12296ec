"""Drop-in for the reference's Cython extension module ``ctc_fast``
(``ctc_fast/ctc-loss/ctc_fast.pyx``, built by ``ctc_fast/ctc-loss/setup.py:7-8``),
running the alpha/beta recursion and the gradient on the MI355X through
libsctc_hip.so.  Same surface, same argument checking, same return values:

    ctc_loss(params, seq, blank=0) -> (cost, grad, skip)      ctc_fast.pyx:13-152
    decode_best_path(probs, blank=0) -> (hyp, align)          ctc_fast.pyx:154-187

``params``/``probs`` are float64 (A, T) Fortran-ordered NumPy arrays and ``seq`` a
C-contiguous int32 vector, exactly what the Cython memoryview signature accepts;
anything else raises ``ValueError`` like the memoryview does.  The float64 host
signature runs the float64 device kernels.  Additional entry points (not in the
reference) take batches and device tensors: :func:`ctc_loss_batch`; and the prefix beam
search decoder of ``ctc_fast/new_decoder/decoder.pyx`` batched over utterances:
:func:`decode_beam_batch` with an optional character LM (an n-gram :class:`DecodeLM`, a
neural :class:`DecodeNNLM` or a recurrent :class:`DecodeRNNLM`); and scoring: :func:`edit_distance_batch` (the table and
trace-back of ``ctc_fast/editDistance.py`` and ``swbd-utils/editDist.pyx`` for many pairs in
one launch), :func:`nbest_oracle`, and the forced alignment :func:`align_batch` with
:func:`score_sentences` (the ``align`` and ``refScore`` of ``decoder_utils.decode``); and the
best path of a whole batch in one launch, :func:`decode_best_path_batch`, with :func:`log_rows` and
:func:`edit_distance_device` for data that stays on the device.

There is no CPU fallback: without the HIP library or without a GPU the calls raise.
"""
import ctypes

import numpy as np

import _sctc

# ctc_fast.pyx:6 -- the reference flips NumPy's error state process-wide at import
np.seterr(divide='raise', invalid='raise')


def _check_params(params, name="params"):
    if params is None:
        raise TypeError("Argument '%s' must not be None" % name)
    if not isinstance(params, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray)" % name)
    if params.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % params.ndim)
    if params.dtype != np.float64:
        raise ValueError("Buffer dtype mismatch, expected 'double' but got '%s'" % params.dtype)
    if not params.flags.f_contiguous:
        raise ValueError("ndarray is not Fortran contiguous")


def _check_seq(seq):
    if seq is None:
        raise TypeError("Argument 'seq' must not be None")
    if not isinstance(seq, np.ndarray):
        raise TypeError("Argument 'seq' has incorrect type (expected numpy.ndarray)")
    if seq.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % seq.ndim)
    if seq.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int' but got '%s'" % seq.dtype)
    if not seq.flags.c_contiguous:
        raise ValueError("ndarray is not C-contiguous")


def _run_batch(probs_dev, grad_dev, A, ld, blank, T_b, U_b, frame_off, labels, label_off,
               dtype, rowbase_dev=None):
    """probs_dev/grad_dev: torch CUDA tensors [rows][ld]; returns (cost, skip) torch tensors."""
    torch = _sctc.require_gpu()
    L = _sctc.lib()
    B = len(T_b)
    T_b = np.ascontiguousarray(T_b, dtype=np.int32)
    U_b = np.ascontiguousarray(U_b, dtype=np.int32)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    label_off = np.ascontiguousarray(label_off, dtype=np.int64)
    bt = _sctc.CtcBatch(B, int(A), int(blank), dtype, int(ld), _sctc.i32(T_b), _sctc.i32(U_b),
                        _sctc.i64(frame_off), _sctc.i32(labels), _sctc.i64(label_off),
                        ctypes.c_void_p(rowbase_dev.data_ptr() if rowbase_dev is not None else 0))
    nbytes = L.sctc_ctc_workspace_bytes(ctypes.byref(bt))
    if nbytes == 0:
        _sctc.check(-1, "ctc_loss")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=probs_dev.device)
    cost = torch.empty(B, dtype=torch.float64, device=probs_dev.device)
    skip = torch.empty(B, dtype=torch.int32, device=probs_dev.device)
    rc = L.sctc_ctc_loss_batch(ctypes.byref(bt), probs_dev.data_ptr(), grad_dev.data_ptr(),
                               cost.data_ptr(), skip.data_ptr(), ws.data_ptr(), nbytes,
                               _sctc.current_stream_ptr())
    _sctc.check(rc, "ctc_loss")
    return cost, skip


def ctc_loss(params, seq, blank=0):
    """CTC loss function (ctc_fast.pyx:13-152).

    params - n x m matrix of n-D probability distributions over m frames, float64,
    Fortran order.  seq - int32 label ids.  Returns (cost, grad, skip): the negative
    log-likelihood, its gradient with respect to the *unnormalised* (pre-softmax)
    activations as a fresh float64 (n, m) Fortran array, and the skip flag the
    reference sets when a frame normaliser is zero (ctc_fast.pyx:147-149).
    """
    _check_params(params)
    _check_seq(seq)
    torch = _sctc.require_gpu()
    A, T = params.shape
    if seq.shape[0] == 0:
        # undefined behaviour in the reference (reads seq[0] out of bounds, ctc_fast.pyx:43)
        raise ValueError("ctc_loss: empty label sequence")
    blank = int(blank)
    if blank < 0:
        raise OverflowError("can't convert negative value to unsigned int")
    dev_probs = torch.from_numpy(params.T).cuda()          # (T, A) row-major == (A,T) F-order
    dev_grad = torch.empty_like(dev_probs)
    cost, skip = _run_batch(dev_probs, dev_grad, A, A, blank, [T], [seq.shape[0]], [0], seq, [0],
                            _sctc.F64)
    grad = np.asfortranarray(dev_grad.cpu().numpy().T)
    return float(cost.item()), grad, bool(skip.item())


def ctc_loss_batch(probs, seqs, blank=0, lengths=None):
    """Batched form (not in the reference).

    probs: list of (A, T_b) float64/float32 F-ordered arrays, or a torch CUDA tensor
    [sum T][A] (float32/float64) with ``lengths`` giving T_b.  Returns
    (cost float64[B], grad in the input's form, skip bool[B]).
    """
    torch = _sctc.require_gpu()
    B = len(seqs)
    U_b = [len(s) for s in seqs]
    labels = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs])
    label_off = np.concatenate([[0], np.cumsum(U_b)[:-1]])
    as_list = not isinstance(probs, torch.Tensor)
    if as_list:
        dt = probs[0].dtype
        T_b = [p.shape[1] for p in probs]
        A = probs[0].shape[0]
        host = np.concatenate([np.ascontiguousarray(np.asarray(p).T) for p in probs], axis=0)
        dev = torch.from_numpy(host).cuda()
    else:
        dev = probs.contiguous()
        T_b = list(lengths)
        A = dev.shape[1]
        dt = np.float64 if dev.dtype == torch.float64 else np.float32
    if dev.dtype not in (torch.float32, torch.float64):
        raise ValueError("Buffer dtype mismatch, expected 'double' or 'float'")
    frame_off = np.concatenate([[0], np.cumsum(T_b)[:-1]])
    grad = torch.empty_like(dev)
    cost, skip = _run_batch(dev, grad, A, dev.shape[1], blank, T_b, U_b, frame_off, labels,
                            label_off, _sctc.F64 if dev.dtype == torch.float64 else _sctc.F32)
    if as_list:
        g = grad.cpu().numpy()
        grads = [np.asfortranarray(g[o:o + t].T.astype(dt)) for o, t in zip(frame_off, T_b)]
        return cost.cpu().numpy(), grads, skip.cpu().numpy().astype(bool)
    return cost, grad, skip.bool()


def decode_best_path(probs, blank=0):
    """Best path decoding (ctc_fast.pyx:154-187): most likely label per frame
    (argmax on the GPU), then drop blanks, drop the reference's hard-coded ids
    1, 2 and 8 (ctc_fast.pyx:176-179), collapse repeats.  Returns (hyp, align)."""
    _check_params(probs, "probs")
    torch = _sctc.require_gpu()
    A, T = probs.shape
    dev = torch.from_numpy(probs.T).cuda()
    best = torch.empty(T, dtype=torch.int32, device=dev.device)
    rc = _sctc.lib().sctc_argmax_rows(dev.data_ptr(), _sctc.F64, best.data_ptr(), T, A, A,
                                      _sctc.current_stream_ptr())
    _sctc.check(rc, "decode_best_path")
    return collapse_best_path(best.cpu().numpy(), blank)


def collapse_best_path(best_path, blank=0):
    hyp, align = [], []
    for i in range(len(best_path)):
        b = int(best_path[i])
        if b == blank:
            continue
        if b == 1 or b == 2 or b == 8:
            continue
        elif i != 0 and b == best_path[i - 1]:
            align[-1] = i
            continue
        else:
            hyp.append(b)
            align.append(i)
    return hyp, align


def decode_best_path_batch(probs, lengths=None, blank=0, drop=(1, 2, 8), spans=False, scores=False, device=False):
    """Best path decoding of a batch in one launch: :func:`decode_best_path` for every
    utterance at once -- arg-max per frame, collapse of repeats, ``blank`` and the ids of ``drop`` never emitted
    (the default is the reference's hard-coded 1, 2, 8 of ctc_fast.pyx:176-179; a dropped symbol still
    separates two runs of one symbol).

    probs: as for :func:`decode_beam_batch` -- a list of (A, T_b) float32/float64 arrays, or a torch device
    tensor [sum T][A] (any row stride) with ``lengths``; probabilities or log-probabilities.  ``blank=None``
    drops nothing but ``drop``.  Returns (hyps, aligns), lists of int32 arrays: the labels, and the last frame
    of each label (what ``decode_best_path`` returns for one utterance).  ``spans=True``: int32 [U, 2] arrays
    (first, last frame) in place of aligns.  ``scores=True``: a third value, float64 [B], the sum of the arg-max
    entries.  ``device=True``: nothing is read back; returns the device tensors (ids int32 [sum T] with the
    labels of utterance b from sum_{q<b} T_q, lens int32 [B], spans int32 [sum T, 2] or None, scores float64
    [B] or None)."""
    what = "decode_best_path_batch"
    arrs, src, A, T_b, dt, dtype = _decode_inputs(probs, lengths, what)
    B = len(T_b)
    never = sorted(set(([] if blank is None else [int(blank)]) + [int(d) for d in drop]))
    if len(never) > _sctc.BESTPATH_MAX_DROP:
        raise ValueError("%s: %d symbols to drop, the limit is %d" % (what, len(never), _sctc.BESTPATH_MAX_DROP))
    torch = _sctc.require_gpu()
    ld = int(A)
    if src is None:
        host = np.concatenate([np.ascontiguousarray(p.T, dtype=dt) for p in arrs], axis=0) if sum(T_b) else \
            np.zeros((1, A), dtype=dt)
        dev = torch.from_numpy(host).cuda()
    else:       # rows of a wider tensor are read in place (ld > A)
        dev = src if src.stride(1) == 1 and src.stride(0) >= A else src.contiguous()
        ld = int(dev.stride(0))
    Tb = np.ascontiguousarray(T_b, dtype=np.int32)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(T_b)[:-1]]) if B else [], dtype=np.int64)
    cfg = _sctc.BestPathConfig(B, int(A), dtype, len(never), (ctypes.c_int32 * 16)(*never), ld, _sctc.i32(Tb),
                               _sctc.i64(off))
    sum_T = int(Tb.sum())
    want_spans = bool(spans) or not device
    ids = torch.empty(max(1, sum_T), dtype=torch.int32, device=dev.device)
    lens = torch.empty(max(1, B), dtype=torch.int32, device=dev.device)[:B]
    span = torch.empty((max(1, sum_T), 2), dtype=torch.int32, device=dev.device) if want_spans else None
    score = torch.empty(max(1, B), dtype=torch.float64, device=dev.device)[:B] if scores else None
    rc = _sctc.lib().sctc_ctc_bestpath_batch(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                             span.data_ptr() if want_spans else None,
                                             score.data_ptr() if scores else None, _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    if device:
        return ids, lens, span, score
    lens_h = lens.cpu().numpy()
    ids_h, span_h = ids.cpu().numpy(), span.cpu().numpy()
    hyps = [ids_h[o:o + n].copy() for o, n in zip(off, lens_h)]
    if spans:
        second = [span_h[o:o + n].copy() for o, n in zip(off, lens_h)]
    else:
        second = [span_h[o:o + n, 1].copy() for o, n in zip(off, lens_h)]
    if scores:
        return hyps, second, score.cpu().numpy()
    return hyps, second


def log_rows(probs_dev, out=None):
    """``(float) log((double) p)`` of a float32 device tensor [rows][A] (any row stride), element by element
    on the device (``sctc_log_rows``): what ``writeLikelihoods.py`` computes on the host.  ``out`` may be the
    input itself (in place); default: a new tensor.  p == 0 gives -inf."""
    torch = _sctc.require_gpu()
    if not (isinstance(probs_dev, torch.Tensor) and probs_dev.is_cuda and probs_dev.dtype == torch.float32
            and probs_dev.dim() == 2 and (probs_dev.shape[1] == 0 or probs_dev.stride(1) == 1)
            and probs_dev.stride(0) >= probs_dev.shape[1]):
        raise ValueError("log_rows: a float32 [rows][A] device tensor with unit column stride expected")
    if out is None:
        out = torch.empty_strided(probs_dev.shape, probs_dev.stride(), dtype=torch.float32, device=probs_dev.device)
    if tuple(out.shape) != tuple(probs_dev.shape) or out.stride() != probs_dev.stride() or out.dtype != torch.float32:
        raise ValueError("log_rows: out must have the input's shape, strides and dtype")
    rows, A = int(probs_dev.shape[0]), int(probs_dev.shape[1])
    if rows and A:
        rc = _sctc.lib().sctc_log_rows(probs_dev.data_ptr(), out.data_ptr(), rows, A, int(probs_dev.stride(0)),
                                       _sctc.current_stream_ptr())
        _sctc.check(rc, "log_rows")
    return out


class _DeviceHandle(object):
    """``handle`` of a device object of the library, destroyed once by the function ``_destroy`` names"""

    _destroy = None
    handle = None

    def close(self):
        if self.handle is not None and self.handle.value:
            getattr(_sctc.lib(), self._destroy)(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecodeLM(_DeviceHandle):
    """A character n-gram LM on the device for :func:`decode_beam_batch`: an
    :class:`arpa_lm.ArpaLM` (or the path of an ARPA file) packed and uploaded once, plus
    the LM word of every CTC symbol -- ``symbols`` is the decoder's ``int_char_map``
    ({symbol id: token}, chars.txt) or an int32 array of word ids per symbol."""

    _destroy = "sctc_lm_destroy"

    def __init__(self, arpa, symbols, A=None):
        import arpa_lm
        if not isinstance(arpa, arpa_lm.ArpaLM):
            arpa = arpa_lm.ArpaLM(arpa)
        self.arpa = arpa
        if isinstance(symbols, dict):
            A = int(A) if A is not None else max(symbols) + 1
            self.sym_words = arpa.symbol_words(symbols, A)
        else:
            self.sym_words = np.ascontiguousarray(symbols, dtype=np.int32)
        self.handle = None
        keys, prob, bo = arpa.pack()
        _sctc.require_gpu()
        h = ctypes.c_void_p()
        rc = _sctc.lib().sctc_lm_create(keys.ctypes.data, prob.ctypes.data, bo.ctypes.data, keys.shape[0],
                                        arpa.order, arpa.bos, ctypes.byref(h))
        _sctc.check(rc, "DecodeLM")
        self.handle = h


class DecodeNNLM(_DeviceHandle):
    """A neural character LM on the device for :func:`decode_beam_batch`: an
    :class:`nn_lm.NNCharLM` (or the path of its ``.npz``) uploaded once, plus the LM id of every
    CTC symbol -- ``symbols`` is the decoder's ``int_char_map`` ({symbol id: token}, chars.txt) or
    an int32 array of LM ids per symbol.  Every symbol 1..A-1 must have an id (ValueError)."""

    _destroy = "sctc_nnlm_destroy"

    def __init__(self, nnlm, symbols, A=None):
        import nn_lm
        if not isinstance(nnlm, nn_lm.NNCharLM):
            nnlm = nn_lm.NNCharLM.load(nnlm)
        self.nnlm = nnlm
        self.handle = None
        if isinstance(symbols, dict):
            A = int(A) if A is not None else max(symbols) + 1
            self.sym_words = nnlm.symbol_words(symbols, A)
        else:
            self.sym_words = np.ascontiguousarray(symbols, dtype=np.int32)
            if A is not None:
                self.sym_words = self.sym_words[:int(A)]
            bad = [c for c in range(1, self.sym_words.shape[0]) if not 0 <= self.sym_words[c] < nnlm.V]
            if bad:
                raise ValueError("DecodeNNLM: symbol %d maps to LM id %d outside the vocabulary"
                                 % (bad[0], self.sym_words[bad[0]]))
        widths, ws, bs = nnlm.padded()
        n = len(ws)
        _sctc.require_gpu()
        wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        h = ctypes.c_void_p()
        rc = _sctc.lib().sctc_nnlm_create(nnlm.V, nnlm.context, n, _sctc.i32(widths), wp, bp, nnlm.bos, nnlm.null,
                                          ctypes.byref(h))
        _sctc.check(rc, "DecodeNNLM")
        self.handle = h
        self.device_bytes = int(_sctc.lib().sctc_nnlm_bytes(h))

    def contexts(self, prefixes):
        """int32 [n, K]: the LM's window of every prefix (a sequence of CTC symbol ids)"""
        out = np.empty((len(prefixes), self.nnlm.context), dtype=np.int32)
        for i, P in enumerate(prefixes):
            out[i] = self.nnlm.context_ids([self.sym_words[int(s)] for s in P])
        return out

    def lm_rows(self, contexts):
        """float32 [n, V]: log10 P(. | context) for int32 [n, K] windows of LM ids"""
        torch = _sctc.require_gpu()
        ctx = np.ascontiguousarray(contexts, dtype=np.int32).reshape(-1, self.nnlm.context)
        if ctx.size and (ctx.min() < 0 or ctx.max() >= self.nnlm.V):
            raise ValueError("DecodeNNLM: a context id outside the vocabulary")
        n = ctx.shape[0]
        dev = torch.from_numpy(ctx).cuda()
        out = torch.empty((n, self.nnlm.V), dtype=torch.float32, device=dev.device)
        rc = _sctc.lib().sctc_nnlm_rows(self.handle, dev.data_ptr(), n, out.data_ptr(), _sctc.current_stream_ptr())
        _sctc.check(rc, "DecodeNNLM.rows")
        return out.cpu().numpy()

    def rows(self, prefixes):
        """float32 [n, A] as the search sees them: column 0 is 0, column c is log10 P(symbol c |
        prefix) for every prefix (a sequence of CTC symbol ids)"""
        r = self.lm_rows(self.contexts(prefixes))
        out = r[:, self.sym_words]
        out[:, 0] = 0.0
        return np.ascontiguousarray(out)


class DecodeRNNLM(_DeviceHandle):
    """A recurrent character LM on the device for :func:`decode_beam_batch`: an
    :class:`nn_lm.RNNCharLM` (or the path of its ``.npz``) uploaded once, plus the LM id of every CTC
    symbol -- ``symbols`` as for :class:`DecodeNNLM`.  Every symbol 1..A-1 must have an id (ValueError)."""

    _destroy = "sctc_rnnlm_destroy"

    def __init__(self, rnnlm, symbols, A=None):
        import nn_lm
        if not isinstance(rnnlm, nn_lm.RNNCharLM):
            rnnlm = nn_lm.RNNCharLM.load(rnnlm)
        self.rnnlm = rnnlm
        self.handle = None
        if isinstance(symbols, dict):
            A = int(A) if A is not None else max(symbols) + 1
            self.sym_words = rnnlm.symbol_words(symbols, A)
        else:
            self.sym_words = np.ascontiguousarray(symbols, dtype=np.int32)
            if A is not None:
                self.sym_words = self.sym_words[:int(A)]
            bad = [c for c in range(1, self.sym_words.shape[0]) if not 0 <= self.sym_words[c] < rnnlm.V]
            if bad:
                raise ValueError("DecodeRNNLM: symbol %d maps to LM id %d outside the vocabulary"
                                 % (bad[0], self.sym_words[bad[0]]))
        self.Hp, Wx, Wh, bh, Wo = rnnlm.padded()
        _sctc.require_gpu()
        h = ctypes.c_void_p()
        rc = _sctc.lib().sctc_rnnlm_create(rnnlm.V, self.Hp, Wx.ctypes.data, Wh.ctypes.data, bh.ctypes.data,
                                           Wo.ctypes.data, rnnlm.bo.ctypes.data, rnnlm.bos, ctypes.byref(h))
        _sctc.check(rc, "DecodeRNNLM")
        self.handle = h
        self.device_bytes = int(_sctc.lib().sctc_rnnlm_bytes(h))

    def step(self, ids, state_in=None, rows=True):
        """One recurrent step on device tensors: ids int32 [n], state_in float32 [n, Hp] or None (zero
        states) -> (state_out [n, Hp], rows [n, V] or None)"""
        torch = _sctc.require_gpu()
        if not (isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1
                and ids.is_contiguous()):
            raise ValueError("DecodeRNNLM.step: ids must be a contiguous int32 [n] tensor on the device")
        n = int(ids.shape[0])
        if state_in is not None and not (isinstance(state_in, torch.Tensor) and state_in.device == ids.device
                                         and state_in.dtype == torch.float32 and state_in.is_contiguous()
                                         and tuple(state_in.shape) == (n, self.Hp)):
            raise ValueError("DecodeRNNLM.step: state_in must be a contiguous float32 [%d, %d] tensor on the device of "
                             "ids, or None" % (n, self.Hp))
        out = torch.empty((n, self.Hp), dtype=torch.float32, device=ids.device)
        r = torch.empty((n, self.rnnlm.V), dtype=torch.float32, device=ids.device) if rows else None
        rc = _sctc.lib().sctc_rnnlm_step(self.handle, ids.data_ptr(), state_in.data_ptr() if state_in is not None else None,
                                         n, out.data_ptr(), r.data_ptr() if rows else None,
                                         _sctc.current_stream_ptr())
        _sctc.check(rc, "DecodeRNNLM.step")
        return out, r

    def _evaluate(self, prefixes, cache=None):
        """[(state [Hp] on the device, LM row [V] on the host)] of prefixes (sequences of CTC symbol ids):
        every distinct prefix, and every prefix of it, is evaluated once, one step call per prefix
        depth.  ``cache``: a dict of the caller's that keeps what was evaluated from call to call."""
        torch = _sctc.require_gpu()
        want = [tuple(int(s) for s in P) for P in prefixes]
        known = cache if cache is not None else {}
        levels = []
        for P in want:
            if any(not 1 <= s < self.sym_words.shape[0] for s in P):
                raise ValueError("DecodeRNNLM: a prefix holds a symbol outside 1..%d" % (self.sym_words.shape[0] - 1))
            for d in range(len(P), -1, -1):
                if P[:d] in known:
                    break
                while len(levels) <= d:
                    levels.append({})
                levels[d].setdefault(P[:d], None)
        for d, level in enumerate(levels):
            todo = list(level)
            if not todo:
                continue
            if d == 0:
                ids, state_in = [self.rnnlm.bos], None
            else:
                ids = [self.sym_words[P[-1]] for P in todo]
                state_in = torch.stack([known[P[:-1]][0] for P in todo])
            out, rows = self.step(torch.from_numpy(np.asarray(ids, dtype=np.int32)).cuda(), state_in)
            rows = rows.cpu().numpy()
            for i, P in enumerate(todo):
                known[P] = (out[i], rows[i])
        return [known[P] for P in want]

    def states(self, prefixes, cache=None):
        """float32 [n, H]: the hidden state of every prefix (a sequence of CTC symbol ids)"""
        torch = _sctc.require_gpu()
        got = self._evaluate(prefixes, cache)
        if not got:
            return np.zeros((0, self.rnnlm.H), dtype=np.float32)
        return np.ascontiguousarray(torch.stack([s for s, _ in got]).cpu().numpy()[:, :self.rnnlm.H])

    def lm_rows(self, prefixes, cache=None):
        """float32 [n, V]: log10 P(. | <s> prefix) by LM id"""
        got = self._evaluate(prefixes, cache)
        return np.stack([r for _, r in got]) if got else np.zeros((0, self.rnnlm.V), dtype=np.float32)

    def rows(self, prefixes, cache=None):
        """float32 [n, A] as the search sees them: column 0 is 0, column c is log10 P(symbol c |
        prefix) for every prefix (a sequence of CTC symbol ids of any length).  Distinct prefixes are
        evaluated once, one step call per prefix depth; with ``cache`` (a dict of the caller's) the
        states of evaluated prefixes are kept from call to call."""
        out = self.lm_rows(prefixes, cache)[:, self.sym_words]
        out[:, 0] = 0.0
        return np.ascontiguousarray(out)


def _decode_inputs(logprobs, lengths, what):
    """(host arrays or None, device tensor or None, A, T_b, numpy dtype, sctc dtype) of a decode call"""
    import torch
    if isinstance(logprobs, torch.Tensor):
        if lengths is None:
            raise ValueError("%s: a device tensor needs lengths" % what)
        if logprobs.dim() != 2:
            raise ValueError("%s: expected a [sum T][A] tensor" % what)
        T_b = [int(t) for t in lengths]
        A = int(logprobs.shape[1])
        if logprobs.dtype not in (torch.float32, torch.float64):
            raise ValueError("Buffer dtype mismatch, expected 'double' or 'float'")
        dtype = _sctc.F64 if logprobs.dtype == torch.float64 else _sctc.F32
        if sum(T_b) > logprobs.shape[0]:
            raise ValueError("%s: lengths exceed the tensor's rows" % what)
        return None, logprobs, A, T_b, None, dtype
    arrs = [np.asarray(p) for p in logprobs]
    if not arrs:
        raise ValueError("%s: empty batch" % what)
    for p in arrs:
        if p.ndim != 2 or p.shape[0] != arrs[0].shape[0]:
            raise ValueError("%s: every utterance must be an (A, T) array of one A" % what)
    A = arrs[0].shape[0]
    T_b = [p.shape[1] for p in arrs]
    dt = np.float64 if any(p.dtype == np.float64 for p in arrs) else np.float32
    return arrs, None, A, T_b, dt, _sctc.F64 if dt == np.float64 else _sctc.F32


def _decode_launch(cfg, bytes_fn, decode_fn, arrs, src, A, T_b, dt, nbest, what, device=False):
    """workspace, upload, launch and read-back shared by the two beam searches; ``device``: no read-back, the
    device tensors (ids, lens, scores) are returned as the search wrote them"""
    B = len(T_b)
    nbytes = bytes_fn(ctypes.byref(cfg))
    if nbytes == 0:
        _sctc.check(-1, what)
    torch = _sctc.require_gpu()
    if src is None:
        host = np.concatenate([np.ascontiguousarray(p.T, dtype=dt) for p in arrs], axis=0) if sum(T_b) else \
            np.zeros((1, A), dtype=dt)
        dev = torch.from_numpy(host).cuda()
    else:
        dev = src.contiguous()
        cfg.ld = int(dev.stride(0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev.device)
    ids = torch.zeros(max(1, nbest * sum(T_b)), dtype=torch.int32, device=dev.device)
    lens = torch.empty(B * nbest, dtype=torch.int32, device=dev.device)
    scores = torch.empty(B * nbest, dtype=torch.float64, device=dev.device)
    rc = decode_fn(ctypes.byref(cfg), dev.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                   scores.data_ptr(), ws.data_ptr(), nbytes, _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    if device:
        return ids, lens, scores
    ids, lens, scores = ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()
    hyps = []
    base = 0
    for b in range(B):
        row = []
        for n in range(nbest):
            o = base + n * T_b[b]
            row.append(ids[o:o + lens[b * nbest + n]].copy())
        hyps.append(row)
        base += nbest * T_b[b]
    if nbest == 1:
        return [h[0] for h in hyps], scores
    return hyps, scores.reshape(B, nbest)


def decode_beam_batch(logprobs, lengths=None, beam=40, alpha=1.0, beta=0.0, lm=None, nbest=1, device=False):
    """CTC prefix beam search with an optional character LM, batched: the
    reference's ``BeamLMDecoder.decode`` (ctc_fast/new_decoder/decoder.pyx:136-193) for every
    utterance at once, one workgroup per utterance.

    logprobs: list of (A, T_b) float32/float64 natural-log probability arrays (symbol 0 the
    blank), or a torch device tensor [sum T][A] with ``lengths`` giving T_b.  lm: a
    :class:`DecodeLM`, a :class:`DecodeNNLM`, a :class:`DecodeRNNLM` (§4.10) or None (no LM term).  Returns (hyps, scores): with nbest == 1 a list
    of int32 symbol-id arrays and float64[B]; with nbest > 1 a list of lists and [B, nbest]
    (entries beyond the beam: empty, -inf).  ``device=True``: nothing is read back; returns the device tensors
    (ids int32 [nbest * sum T], rank n of utterance b from nbest * sum_{q<b} T_q + n * T_b; lens int32
    [B * nbest]; scores float64 [B * nbest])."""
    arrs, src, A, T_b, dt, dtype = _decode_inputs(logprobs, lengths, "decode_beam_batch")
    B = len(T_b)
    search = [(cfg, name) for kind, cfg, name in _BEAM_SEARCH if isinstance(lm, kind)]
    if not search:
        raise ValueError("decode_beam_batch: lm must be a ctc_fast.DecodeLM, a ctc_fast.DecodeNNLM, a "
                         "ctc_fast.DecodeRNNLM or None")
    config, name = search[0]
    if lm is not None and lm.sym_words.shape[0] < A:
        raise ValueError("decode_beam_batch: the LM maps %d symbols, the input has %d"
                         % (lm.sym_words.shape[0], A))
    Tb = np.ascontiguousarray(T_b, dtype=np.int32)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(T_b)[:-1]]) if B else [], dtype=np.int64)
    sw = np.ascontiguousarray(lm.sym_words[:A] if lm is not None else np.zeros(A, np.int32), dtype=np.int32)
    cfg = config(B, int(A), dtype, int(beam), int(nbest), 0, int(A), _sctc.i32(Tb), _sctc.i64(off), float(alpha),
                 float(beta), lm.handle if lm is not None else None, _sctc.i32(sw))
    L = _sctc.lib()
    return _decode_launch(cfg, getattr(L, "sctc_ctc_%s_workspace_bytes" % name),
                          getattr(L, "sctc_ctc_%s_decode_batch" % name), arrs, src, A, T_b, dt, nbest,
                          "decode_beam_batch", device=device)


# decode_beam_batch by the type of its LM: the config class and the name of the entry points
_BEAM_SEARCH = (((DecodeLM, type(None)), _sctc.BeamConfig, "beam"),
                (DecodeNNLM, _sctc.NNBeamConfig, "nnbeam"),
                (DecodeRNNLM, _sctc.RNNBeamConfig, "rnnbeam"))


class DecodeLexicon(_DeviceHandle):
    """A lexicon on the device for :func:`decode_lexicon_beam_batch`: the prefix tree of
    ``words`` (plus ``specials``, tokens that are whole words) and the word-bigram LM ``arpa``
    (a :class:`decoder.lm.LM` or the path of an ARPA file), flattened and uploaded once.

    order: 2 (the default) with a path or an ``LM`` is the word-bigram LM of DESIGN.md §4.6; 3..5 with
    a path reads the file as a :class:`decoder.ngram_lm.NgramLM` of that order (§4.6b), and an
    ``NgramLM`` given as ``arpa`` is used at its own order, 2 included: with one, ``order`` is left at
    its default or names the LM's own order, anything else is a ``ValueError``.

    chars: {token: symbol id} or the path of a ``token id`` file; words: a list or the path of a
    word list; space: the separator token or its symbol id; A: the alphabet size of the inputs
    (default: the largest symbol id + 1)."""

    _destroy = "sctc_lexicon_destroy"

    def __init__(self, words, chars, arpa, space, specials=(), A=None, order=2):
        from decoder import decoder_utils, lm as lm_mod, ngram_lm, prefixTree
        order = int(order)
        if not ngram_lm.MIN_ORDER <= order <= ngram_lm.MAX_ORDER:
            raise ValueError("DecodeLexicon: order %d outside %d..%d" % (order, ngram_lm.MIN_ORDER, ngram_lm.MAX_ORDER))
        if isinstance(arpa, lm_mod.LM) and order != 2:
            raise ValueError("DecodeLexicon: a decoder.lm.LM holds bigrams only; order %d needs a path or an NgramLM"
                             % order)
        if isinstance(arpa, ngram_lm.NgramLM) and order not in (2, arpa.order):
            raise ValueError("DecodeLexicon: order %d asked, the NgramLM was read at order %d" % (order, arpa.order))
        if isinstance(chars, str):
            chars = decoder_utils.load_chars(chars)
        if isinstance(words, str):
            words = decoder_utils.load_words(words)
        if not isinstance(arpa, (lm_mod.LM, ngram_lm.NgramLM)):
            arpa = lm_mod.LM(arpa) if order == 2 else ngram_lm.NgramLM(arpa, order)
        tree = prefixTree.PrefixTree(chars, words, arpa, specials=specials, space=space)
        self.handle = None
        self._upload(tree, arpa, int(A) if A is not None else max(chars.values()) + 1)

    @classmethod
    def from_tree(cls, tree, lm, A):
        """from a built :class:`decoder.prefixTree.PrefixTree` and its LM, a :class:`decoder.lm.LM` or a
        :class:`decoder.ngram_lm.NgramLM`"""
        self = cls.__new__(cls)
        self.handle = None
        self._upload(tree, lm, int(A))
        return self

    def _upload(self, tree, lm, A):
        from decoder import ngram_lm
        self.tree, self.lm, self.A, self.space = tree, lm, A, int(tree.space)
        child, word = tree.flatten(A)
        self.order = lm.order if isinstance(lm, ngram_lm.NgramLM) else 2
        table = lm.pack() if isinstance(lm, ngram_lm.NgramLM) else lm.pack_bigrams()
        self.nodes = child.shape[0]
        _sctc.require_gpu()
        h = ctypes.c_void_p()
        ug = np.ascontiguousarray(lm.ug, dtype=np.float32)
        bo = np.ascontiguousarray(lm.bo, dtype=np.float32)
        tree_args = (child.ctypes.data, word.ctypes.data, child.shape[0], A, self.space, ug.ctypes.data,
                     bo.ctypes.data, ug.shape[0])
        if isinstance(lm, ngram_lm.NgramLM):
            keys, vals, bos, ids, contexts = table
            rc = _sctc.lib().sctc_lexicon_create_ngram(*(tree_args + (keys.ctypes.data, vals.ctypes.data, bos.ctypes.data,
                                                                      ids.ctypes.data, keys.shape[0], contexts,
                                                                      lm.order, int(lm.start), ctypes.byref(h))))
        else:
            keys, vals = table
            rc = _sctc.lib().sctc_lexicon_create(*(tree_args + (keys.ctypes.data, vals.ctypes.data, keys.shape[0],
                                                                int(lm.start), ctypes.byref(h))))
        _sctc.check(rc, "DecodeLexicon")
        self.handle = h
        self.device_bytes = int(_sctc.lib().sctc_lexicon_bytes(h))


def decode_lexicon_beam_batch(logprobs, lengths=None, lexicon=None, beam=40, alpha=1.0, beta=0.0, nbest=1,
                              device=False):
    """Lexicon-constrained CTC prefix beam search with a word-bigram LM, or with a word n-gram LM of
    order 2..5 when the lexicon was built with one (§4.6b), batched (DESIGN.md
    §4.6): the reference's ``decode_bg_lm`` (ctc_fast/decoder/bg_decoder.pyx:18-95) for every
    utterance at once, one workgroup per utterance.  Inputs and outputs as
    :func:`decode_beam_batch`; lexicon: a :class:`DecodeLexicon`.  A hypothesis spells lexicon
    words separated by the space symbol and may end inside a word; its score is
    log(p_nb + p_b) + beta * (words finished).  ``device=True`` as for :func:`decode_beam_batch`."""
    if not isinstance(lexicon, DecodeLexicon):
        raise ValueError("decode_lexicon_beam_batch: lexicon must be a ctc_fast.DecodeLexicon")
    arrs, src, A, T_b, dt, dtype = _decode_inputs(logprobs, lengths, "decode_lexicon_beam_batch")
    if A != lexicon.A:
        raise ValueError("decode_lexicon_beam_batch: the lexicon was built for %d symbols, the input has %d"
                         % (lexicon.A, A))
    B = len(T_b)
    Tb = np.ascontiguousarray(T_b, dtype=np.int32)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(T_b)[:-1]]) if B else [], dtype=np.int64)
    cfg = _sctc.LexBeamConfig(B, int(A), dtype, int(beam), int(nbest), lexicon.space, int(A), _sctc.i32(Tb),
                              _sctc.i64(off), float(alpha), float(beta), lexicon.handle)
    L = _sctc.lib()
    return _decode_launch(cfg, L.sctc_ctc_lexbeam_workspace_bytes, L.sctc_ctc_lexbeam_decode_batch, arrs, src, A,
                          T_b, dt, nbest, "decode_lexicon_beam_batch", device=device)


# ---- scoring: edit distance with error counts and alignments ----

OP_MATCH, OP_UP, OP_LEFT, OP_SUB = 0, 1, 2, 3


def _edit_seq(seq, what):
    arr = np.asarray(seq)
    if arr.size == 0:
        return np.zeros(0, dtype=np.int32)
    if arr.ndim != 1 or arr.dtype.kind not in "iub":
        raise ValueError("%s: every sequence must be a 1-d sequence of integers" % what)
    if arr.dtype != np.int32:
        wide = arr.astype(np.int64) if arr.dtype != np.uint64 else arr
        if wide.max() > 2 ** 31 - 1 or wide.min() < -2 ** 31:
            raise ValueError("%s: symbol outside the int32 range" % what)
    if arr.shape[0] > _sctc.EDIT_MAX_LEN:
        raise ValueError("%s: a sequence of %d symbols, the limit is %d" % (what, arr.shape[0], _sctc.EDIT_MAX_LEN))
    return np.ascontiguousarray(arr, dtype=np.int32)


def edit_distance_batch(a_seqs, b_seqs, ops=False, a_index=None):
    """Edit distance, error counts and (``ops=True``) alignments of many pairs of integer
    sequences in one launch: the table and trace-back of ``ctc_fast/editDistance.py:14-45``
    with a = ref, b = hyp, and of ``swbd-utils/editDist.pyx:47-106`` with a = hyp, b = ref.

    a_seqs, b_seqs: lists of integer sequences (any integer dtype, converted to int32, at most
    8191 symbols each), one pair per position.  With ``a_index`` (one entry per element of
    b_seqs) pair p is (a_seqs[a_index[p]], b_seqs[p]): every a is uploaded once however many
    pairs use it (one reference, many hypotheses).

    Returns ``stats``, int32 [P, 5]: distance, UP, LEFT, SUB, MATCH, where UP consumes a symbol
    of a alone and LEFT one of b alone (editDistance's ins / dels, editDist's dels / ins).  With
    ``ops=True`` also a list of int8 arrays, the operations of each pair's path from the start
    of the sequences to their end (OP_MATCH, OP_UP, OP_LEFT, OP_SUB).  One upload, one launch,
    one read-back; distance-only calls use no device workspace."""
    what = "edit_distance_batch"
    a_arr = [_edit_seq(s, what) for s in a_seqs]
    b_arr = [_edit_seq(s, what) for s in b_seqs]
    P = len(b_arr)
    if a_index is None:
        if len(a_arr) != P:
            raise ValueError("%s: %d a sequences for %d b sequences" % (what, len(a_arr), P))
        a_idx = np.arange(P, dtype=np.int64)
    else:
        a_idx = np.asarray(a_index, dtype=np.int64).reshape(-1)
        if a_idx.shape[0] != P or (P and (a_idx.min() < 0 or a_idx.max() >= len(a_arr))):
            raise ValueError("%s: a_index must name one of the %d a sequences for each of the %d pairs"
                             % (what, len(a_arr), P))
    lens_a = np.array([s.shape[0] for s in a_arr], dtype=np.int64)
    lens_b = np.array([s.shape[0] for s in b_arr], dtype=np.int64)
    starts_a = np.concatenate([[0], np.cumsum(lens_a)])[:len(a_arr)].astype(np.int64)
    total_a = int(lens_a.sum())
    a_len = np.ascontiguousarray(lens_a[a_idx] if P else [], dtype=np.int32)
    a_off = np.ascontiguousarray(starts_a[a_idx] if P else [], dtype=np.int64)
    b_len = np.ascontiguousarray(lens_b, dtype=np.int32)
    b_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens_b)])[:P], dtype=np.int64)
    flags = _sctc.EDIT_OPS if ops else 0
    cfg = _sctc.EditConfig(P, flags, _sctc.i32(a_len), _sctc.i64(a_off), _sctc.i32(b_len), _sctc.i64(b_off))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_edit_distance_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), what)
    if P == 0:
        stats = np.zeros((0, 5), dtype=np.int32)
        return (stats, []) if ops else stats
    torch = _sctc.require_gpu()
    host = np.concatenate(a_arr + b_arr + [np.zeros(1, dtype=np.int32)])
    dev = torch.from_numpy(host).cuda()
    path_len = a_len.astype(np.int64) + b_len
    ops_total = int(path_len.sum()) if ops else 0
    # one output buffer, one read-back: [P][5] stats | [P] path lengths | the paths
    out = torch.empty(24 * P + ops_total, dtype=torch.uint8, device=dev.device)
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=dev.device)
    base = out.data_ptr()
    rc = L.sctc_edit_distance_batch(ctypes.byref(cfg), dev.data_ptr(), dev.data_ptr() + 4 * total_a, base,
                                    base + 24 * P if ops else None, base + 20 * P if ops else None,
                                    ws.data_ptr() if nbytes.value else None, nbytes.value,
                                    _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    got = out.cpu().numpy()
    stats = got[:20 * P].view(np.int32).reshape(P, 5).copy()
    if not ops:
        return stats
    lens = got[20 * P:24 * P].view(np.int32)
    codes = got[24 * P:].view(np.int8)
    starts = np.concatenate([[0], np.cumsum(path_len)])
    return stats, [codes[starts[p]:starts[p] + lens[p]].copy() for p in range(P)]


def edit_distance_device(a_dev, a_len, a_off, b_dev, b_len, b_off):
    """:func:`edit_distance_batch` (counts only) for sequences that already lie on the device: pair p is
    (a_dev[a_off[p] : a_off[p] + a_len[p]], b_dev[b_off[p] : b_off[p] + b_len[p]]).  a_dev, b_dev: contiguous
    int32 device tensors; the lengths (0..8191) and offsets are host sequences, one entry per pair.  Returns the
    stats as an int32 [P, 5] DEVICE tensor (distance, UP, LEFT, SUB, MATCH); nothing is read back."""
    what = "edit_distance_device"
    torch = _sctc.require_gpu()
    for t in (a_dev, b_dev):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError("%s: contiguous int32 device tensors expected" % what)
    a_len = np.ascontiguousarray(a_len, dtype=np.int32).reshape(-1)
    b_len = np.ascontiguousarray(b_len, dtype=np.int32).reshape(-1)
    a_off = np.ascontiguousarray(a_off, dtype=np.int64).reshape(-1)
    b_off = np.ascontiguousarray(b_off, dtype=np.int64).reshape(-1)
    P = a_len.shape[0]
    if not (b_len.shape[0] == a_off.shape[0] == b_off.shape[0] == P):
        raise ValueError("%s: lengths and offsets must have one entry per pair" % what)
    for n, o, t in ((a_len, a_off, a_dev), (b_len, b_off, b_dev)):
        if P and (n.min() < 0 or o.min() < 0 or int((o + n).max()) > t.numel()):
            raise ValueError("%s: a sequence outside its tensor" % what)
    stats = torch.empty((P, 5), dtype=torch.int32, device=a_dev.device)
    if P == 0:
        return stats
    cfg = _sctc.EditConfig(P, 0, _sctc.i32(a_len), _sctc.i64(a_off), _sctc.i32(b_len), _sctc.i64(b_off))
    rc = _sctc.lib().sctc_edit_distance_batch(ctypes.byref(cfg), a_dev.data_ptr(), b_dev.data_ptr(), stats.data_ptr(),
                                              None, None, None, 0, _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    return stats


# ---- forced alignment and sentence scoring ----

ALIGN_WAVE_MAX_S = 512          # states of the wave path (csrc/ctc_align.hip)
ALIGN_BP_LDS_BYTES = 64 * 1024  # back-pointers of an utterance stay on chip up to this size
ALIGN_STAGE_BYTES = 16 * 1024   # otherwise the trace-back stages them through a block of this size


def align_plan(U_max, path=None):
    """How ctc_align.hip runs a batch whose longest label row has ``U_max`` labels (``path``: the
    value of SCTC_ALIGN_PATH, None = not set): ``path``, states per thread ``spl``, threads ``nl``,
    frames per back-pointer word ``fpw``, ``lds_frames`` (the largest T whose back-pointers stay on
    chip) and ``stage_frames`` (frames per staging block of the trace-back beyond that)."""
    S = 2 * int(U_max) + 1
    wide = S > ALIGN_WAVE_MAX_S or path == "wide"
    if wide:
        spl, nl = 8, max(64, ((S + 7) // 8 + 63) // 64 * 64)
    else:
        spl, nl = (1 if S <= 64 else 2 if S <= 128 else 4 if S <= 256 else 8), 64
    fpw = 16 // spl
    return {"path": "wide" if wide else "wave", "spl": spl, "nl": nl, "fpw": fpw,
            "lds_frames": ALIGN_BP_LDS_BYTES // (4 * nl) * fpw, "stage_frames": ALIGN_STAGE_BYTES // (4 * nl) * fpw}


def align_batch(logprobs, seqs, lengths=None, blank=0, total=False):
    """CTC forced alignment of a label row per utterance, batched: the best path
    of ``seqs[b]`` through the lattice of ctc_fast.pyx:42-76 over utterance b, and with
    ``total=True`` also log P_ctc(seqs[b] | utterance b), the sum over all of its alignments.

    logprobs: as for :func:`decode_beam_batch` -- a list of (A, T_b) float32/float64 natural-log
    probability arrays, or a torch device tensor [sum T][A] (any row stride) with ``lengths``.
    seqs: one integer sequence per utterance, at most 4095 labels.  Returns (frame_label, spans,
    viterbi, total, status): a list of int32 [T_b] (the index u of the label a frame is aligned to,
    -1 for blank), a list of int32 [U_b, 2] (first and last frame of label u, inclusive), float64
    [B], float64 [B] or None, int32 [B] (0 aligned; 1 no alignment of finite score; 2 a label
    outside [0, A) or equal to the blank; then the scores are -inf and the rest -1)."""
    what = "align_batch"
    arrs, src, A, T_b, dt, dtype = _decode_inputs(logprobs, lengths, what)
    B = len(T_b)
    if len(seqs) != B:
        raise ValueError("%s: %d label rows for %d utterances" % (what, len(seqs), B))
    for s in seqs:
        if len(s) > _sctc.ALIGN_MAX_U:
            raise ValueError("%s: a label row of %d labels, the limit is %d" % (what, len(s), _sctc.ALIGN_MAX_U))
    labs = [_edit_seq(s, what) for s in seqs]
    U_b = np.ascontiguousarray([s.shape[0] for s in labs], dtype=np.int32)
    Tb = np.ascontiguousarray(T_b, dtype=np.int32)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(T_b)[:-1]]) if B else [], dtype=np.int64)
    loff = np.ascontiguousarray(np.concatenate([[0], np.cumsum(U_b)[:-1]]) if B else [], dtype=np.int64)
    ld = int(A)
    if src is not None:     # rows of a wider tensor are read in place (ld > A)
        dev = src if src.stride(1) == 1 and A <= src.stride(0) < 2 ** 31 else src.contiguous()
        ld = int(dev.stride(0))
    flags = _sctc.ALIGN_TOTAL if total else 0
    cfg = _sctc.AlignConfig(B, int(A), dtype, int(blank), ld, flags, _sctc.i32(Tb), _sctc.i64(off), _sctc.i32(U_b),
                            _sctc.i64(loff))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), what)
    torch = _sctc.require_gpu()
    if src is None:
        host = np.concatenate([np.ascontiguousarray(p.T, dtype=dt) for p in arrs], axis=0) if sum(T_b) else \
            np.zeros((1, A), dtype=dt)
        dev = torch.from_numpy(host).cuda()
    sum_T, sum_U = int(Tb.sum()), int(U_b.sum())
    labels = torch.from_numpy(np.concatenate(labs + [np.zeros(1, dtype=np.int32)])).to(dev.device)
    # one output buffer, one read-back: [B][2] scores | [B] status | frame labels | spans
    o_status, o_fl, o_span = 16 * B, 20 * B, 20 * B + 4 * sum_T
    out = torch.empty(o_span + 8 * sum_U + 8, dtype=torch.uint8, device=dev.device)
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=dev.device)
    base = out.data_ptr()
    rc = L.sctc_ctc_align_batch(ctypes.byref(cfg), dev.data_ptr(), labels.data_ptr(), base + o_fl, base + o_span, base,
                                base + o_status, ws.data_ptr() if nbytes.value else None, nbytes.value,
                                _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    got = out.cpu().numpy()
    scores = got[:o_status].view(np.float64).reshape(B, 2)
    status = got[o_status:o_fl].view(np.int32).copy()
    fl = got[o_fl:o_span].view(np.int32)
    span = got[o_span:o_span + 8 * sum_U].view(np.int32).reshape(sum_U, 2)
    frame_label = [fl[o:o + t].copy() for o, t in zip(off, T_b)]
    spans = [span[o:o + u].copy() for o, u in zip(loff, U_b)]
    return frame_label, spans, scores[:, 0].copy(), scores[:, 1].copy() if total else None, status


def lm_sentence_scores(seqs, lm):
    """float64 [B]: sum_i log10 P_LM(l_i | <s>, l_<i) of every label row under ``lm`` (a :class:`DecodeLM`,
    a :class:`DecodeNNLM` or a :class:`DecodeRNNLM`), the float32 values that the beam search adds, summed in float64; no
    end-of-sentence term.  An n-gram LM is scored on the host (``ArpaLM.score_ids``), a neural LM by
    one ``rows`` call over all prefixes."""
    out = np.zeros(len(seqs), dtype=np.float64)
    if isinstance(lm, DecodeLM):
        for b, s in enumerate(seqs):
            ctx = [lm.arpa.bos]
            for c in s:
                w = int(lm.sym_words[int(c)])
                out[b] += float(lm.arpa.score_ids(ctx, w))
                ctx.append(w)
        return out
    if not isinstance(lm, (DecodeNNLM, DecodeRNNLM)):
        raise ValueError("lm must be a ctc_fast.DecodeLM, a ctc_fast.DecodeNNLM, a ctc_fast.DecodeRNNLM or None")
    prefixes = [tuple(int(c) for c in s[:i]) for s in seqs for i in range(len(s))]
    if prefixes:
        rows = lm.rows(prefixes)
        k = 0
        for b, s in enumerate(seqs):
            for c in s:
                out[b] += float(rows[k, int(c)])
                k += 1
    return out


def score_sentences(logprobs, seqs, lengths=None, lm=None, alpha=1.0, beta=0.0, word_lm=None, word_alpha=1.0,
                    word_beta=0.0, word_final=True):
    """float64 [B]: the score of label row ``seqs[b]`` under the objective that the character beam
    search maximises, log P_ctc(l) + alpha * sum_i log10 P_LM(l_i | <s>, l_<i) + beta * U: what the
    key of :func:`decode_beam_batch` converges to for prefix l with nothing pruned.
    No end-of-sentence term, as in ``BeamLMDecoder``.  -inf where the row cannot be aligned
    (status != 0 of :func:`align_batch`).  One :func:`align_batch` call; the LM term is computed on
    the host (:func:`lm_sentence_scores`).

    word_lm (a :class:`DecodeLexicon`): adds ``word_alpha * (sum of the word LM's terms) + word_beta * words`` by the
    rules of :func:`word_lm_sentence_scores` (natural log, no ``</s>`` term); a row the word LM cannot score is -inf.
    With ``lm=None, beta=0, word_final=False`` this is the objective of :func:`decode_lexicon_beam_batch` with
    ``alpha=word_alpha, beta=word_beta``."""
    rows = [np.asarray(s).reshape(-1) for s in seqs]
    _, _, _, total, status = align_batch(logprobs, rows, lengths=lengths, total=True)
    score = np.full(len(rows), -np.inf, dtype=np.float64)
    ok = status == 0
    if lm is not None and not isinstance(lm, (DecodeLM, DecodeNNLM, DecodeRNNLM)):
        raise ValueError("score_sentences: lm must be a ctc_fast.DecodeLM, a ctc_fast.DecodeNNLM, a "
                         "ctc_fast.DecodeRNNLM or None")
    good = [r if o else r[:0] for r, o in zip(rows, ok)]
    lmv = lm_sentence_scores(good, lm) if lm is not None else np.zeros(len(rows))
    for b in np.nonzero(ok)[0]:
        score[b] = total[b] + float(alpha) * lmv[b] + float(beta) * len(rows[b])
    if word_lm is not None:
        wsum, wcount, wstatus = word_lm_sentence_scores(good, word_lm, final_word=word_final)
        for b in np.nonzero(ok)[0]:
            score[b] = score[b] + (float(word_alpha) * wsum[b] + float(word_beta) * float(wcount[b, 0])) \
                if wstatus[b] == 0 else -np.inf
    return score


# ---- LM scores on the device and n-best rescoring ----

def _lm_kind(lm, what):
    for kind, cls in ((_sctc.LM_NGRAM, DecodeLM), (_sctc.LM_NN, DecodeNNLM), (_sctc.LM_RNN, DecodeRNNLM)):
        if isinstance(lm, cls):
            return kind
    raise ValueError("%s: lm must be a ctc_fast.DecodeLM, a ctc_fast.DecodeNNLM or a ctc_fast.DecodeRNNLM" % what)


def _lm_score_launch(lm, sym_words, labels_dev, U_b, loff, want_terms, what):
    """sctc_lm_score_batch on device labels: (sums float64 [N], terms float32 [sum U] or None, status int32 [N]),
    device tensors; the workspace is a torch allocation that lives until the stream has run past the call"""
    torch = _sctc.require_gpu()
    kind = _lm_kind(lm, what)
    N = int(U_b.shape[0])
    sw = np.ascontiguousarray(sym_words, dtype=np.int32)
    cfg = _sctc.LmScoreConfig(N, int(sw.shape[0]), kind, 0, lm.handle, _sctc.i32(sw), _sctc.i32(U_b), _sctc.i64(loff))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_lm_score_workspace_bytes(ctypes.byref(cfg), 0 if want_terms else 1, ctypes.byref(nbytes)), what)
    device = labels_dev.device
    sums = torch.empty(N, dtype=torch.float64, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)
    terms = torch.empty(max(1, int(U_b.sum())), dtype=torch.float32, device=device) if want_terms else None
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=device)
    rc = L.sctc_lm_score_batch(ctypes.byref(cfg), labels_dev.data_ptr(), terms.data_ptr() if want_terms else None,
                               sums.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes.value,
                               _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    return sums, (terms[:int(U_b.sum())] if want_terms else None), status


def _score_seqs(seqs, what, max_len):
    """(device labels int32, U_b int32 [N], label_off int64 [N]) of a list of symbol-id arrays, or of a
    device triple (ids, U, offsets) that is read in place"""
    torch = _sctc.require_gpu()
    if isinstance(seqs, tuple) and len(seqs) == 3 and isinstance(seqs[0], torch.Tensor):
        ids, U, offs = seqs
        if not (ids.is_cuda and ids.dtype == torch.int32 and ids.dim() == 1 and ids.is_contiguous()):
            raise ValueError("%s: ids must be a contiguous int32 [n] tensor on the device" % what)
        U_b = np.ascontiguousarray(U.cpu().numpy() if isinstance(U, torch.Tensor) else U, dtype=np.int32).reshape(-1)
        loff = np.ascontiguousarray(offs.cpu().numpy() if isinstance(offs, torch.Tensor) else offs,
                                    dtype=np.int64).reshape(-1)
        if U_b.shape[0] != loff.shape[0]:
            raise ValueError("%s: %d lengths for %d offsets" % (what, U_b.shape[0], loff.shape[0]))
        if U_b.size and ((U_b < 0).any() or (loff < 0).any() or int((loff + U_b).max()) > ids.shape[0]):
            raise ValueError("%s: a sequence lies outside the ids tensor" % what)
        labels = ids
    else:
        labs = [_edit_seq(s, what) for s in seqs]
        U_b = np.ascontiguousarray([s.shape[0] for s in labs], dtype=np.int32)
        loff = np.ascontiguousarray(np.concatenate([[0], np.cumsum(U_b)[:-1]]) if len(labs) else [], dtype=np.int64)
        labels = torch.from_numpy(np.concatenate(labs + [np.zeros(1, dtype=np.int32)])).cuda()
    if U_b.size and int(U_b.max()) > max_len:
        raise ValueError("%s: a sequence of %d labels, the limit is %d" % (what, int(U_b.max()), max_len))
    return labels, U_b, loff


def lm_score_batch(seqs, lm, terms=False, device=False):
    """float64 [N]: sum_i log10 P_LM(l_i | <s>, l_<i) of every label row under ``lm`` (a :class:`DecodeLM`, a
    :class:`DecodeNNLM` or a :class:`DecodeRNNLM`), computed on the device: what
    :func:`lm_sentence_scores` returns, bit for bit, in a few launches for the whole batch.  No end-of-sentence
    term.  ``seqs``: a list of CTC symbol-id sequences, or a device triple (ids int32 tensor, U, offsets) read in
    place -- sequence n is ids[offsets[n] : offsets[n] + U[n]]; offsets may repeat.  A sequence with a symbol
    outside 1..A-1 scores -inf.  ``terms=True``: returns (sums, terms), terms the float32 value of every position
    (a list of arrays; with ``device=True`` one flat tensor, sequence n from sum(U[:n])).  ``device=True``:
    nothing is read back, the results are device tensors."""
    what = "lm_score_batch"
    _lm_kind(lm, what)
    labels, U_b, loff = _score_seqs(seqs, what, _sctc.LM_SCORE_MAX_U)
    sums, tv, _ = _lm_score_launch(lm, lm.sym_words, labels, U_b, loff, bool(terms), what)
    if device:
        return (sums, tv) if terms else sums
    sums = sums.cpu().numpy()
    if not terms:
        return sums
    flat = tv.cpu().numpy()
    cuts = np.concatenate([[0], np.cumsum(U_b)]).astype(np.int64)
    return sums, [flat[cuts[n]:cuts[n + 1]].copy() for n in range(U_b.shape[0])]


def lm_perplexity(seqs_of_lm_ids, lm, eos=True):
    """(perplexity, bits_per_char, n_terms) of sentences given as sequences of LM ids under ``lm`` (a Decode*LM
    handle): 10 ** (-sum of the log10 terms / n), the ``compute_pp`` of the reference's ctc_fast/clm/clm_pp.py.
    Every sentence starts from ``<s>``; with ``eos`` its ``</s>`` term is included.  The LM's ids are scored
    under the identity symbol map (A = V), whatever CTC alphabet the handle was made for; id 0 is the place of
    the blank and cannot be scored (ValueError)."""
    what = "lm_perplexity"
    kind = _lm_kind(lm, what)
    if kind == _sctc.LM_NGRAM:
        V, end = len(lm.arpa.words) + 1, lm.arpa.vocab.get("</s>")
    else:
        model = lm.nnlm if kind == _sctc.LM_NN else lm.rnnlm
        V, end = model.V, model.eos
    if eos and end is None:
        raise ValueError("%s: the LM has no </s>" % what)
    rows = []
    for s in seqs_of_lm_ids:
        r = [int(i) for i in s] + ([int(end)] if eos else [])
        if any(not 1 <= i < V for i in r):
            raise ValueError("%s: an LM id outside 1..%d" % (what, V - 1))
        rows.append(np.asarray(r, dtype=np.int32))
    n = int(sum(r.shape[0] for r in rows))
    if n == 0:
        raise ValueError("%s: nothing to score" % what)
    labels, U_b, loff = _score_seqs(rows, what, _sctc.LM_SCORE_MAX_U)
    sums, _, _ = _lm_score_launch(lm, np.arange(V, dtype=np.int32), labels, U_b, loff, False, what)
    mean = float(sums.cpu().numpy().sum()) / n
    return 10.0 ** (-mean), -mean * np.log2(10.0), n


# ---- the word LM as a second pass ----

def _word_lexicon(lexicon, what):
    if not isinstance(lexicon, DecodeLexicon):
        raise ValueError("%s: the word LM must be a ctc_fast.DecodeLexicon" % what)
    return lexicon


def word_lm_sentence_scores(seqs, lexicon, eos=False, final_word=True):
    """The host route of :func:`word_lm_score_batch` (no GPU): (sums float64 [N], counts int32 [N, 2], status int32
    [N]) of label rows under the word LM of ``lexicon`` -- a :class:`DecodeLexicon`, or anything with its ``tree``
    (a ``PrefixTree``), ``lm`` (a ``decoder.lm.LM`` or a ``decoder.ngram_lm.NgramLM``) and ``A``.

    A token is a maximal run of symbols other than the tree's space (``str.split()``); every token is a word, except
    the last one when no space follows it and ``final_word`` is False (the lexicon search's count).  A token's word id
    is what the tree gives at the end of its spelling; a token that leaves the tree, or ends at no word, is OOV and
    scores as ``lm.unk``.  Term k is ``bg_prob(previous word, w)`` / ``prob(<s> + the words before, w)``, float32,
    NATURAL log; ``eos`` adds ``P(</s> | history)``, which is no word.  The sum is float64 in word order.  counts:
    (words, OOV words).  status: 0; 2 a symbol outside 1..A-1 (sum -inf, counts 0); 3 an OOV word and the LM has no
    ``<UNK>`` (sum -inf)."""
    from decoder import ngram_lm
    tree, lm, A = lexicon.tree, lexicon.lm, int(lexicon.A)
    ngram = isinstance(lm, ngram_lm.NgramLM)
    space = int(tree.space)
    N = len(seqs)
    sums = np.zeros(N, dtype=np.float64)
    counts = np.zeros((N, 2), dtype=np.int32)
    status = np.zeros(N, dtype=np.int32)
    for n, s in enumerate(seqs):
        row = [int(c) for c in np.asarray(s).reshape(-1)]
        if any(not 1 <= c < A for c in row):
            status[n], sums[n] = 2, -np.inf
            continue
        tokens, cur = [], []
        for c in row:
            if c == space:
                if cur:
                    tokens.append(cur)
                cur = []
            else:
                cur.append(c)
        if cur and final_word:
            tokens.append(cur)
        ids = []
        for tok in tokens:
            node = tree.root
            for c in tok:
                node = node.children[c] if node.children is not None and c in node.children else None
                if node is None:
                    break
            known = node is not None and node.isWord
            counts[n, 1] += 0 if known else 1
            ids.append(int(node.id) if known else lm.unk)
        counts[n, 0] = len(ids)
        if any(w is None for w in ids):
            status[n], sums[n] = 3, -np.inf
            continue
        hist = [int(lm.start)]
        total = 0.0
        for w in ids + ([int(lm.end)] if eos else []):
            total += float(lm.prob(hist, w) if ngram else lm.bg_prob(hist[-1], w))
            hist.append(w)
        sums[n] = total
    return sums, counts, status


def _word_lm_launch(lexicon, labels_dev, U_b, loff, want_terms, want_words, eos, final_word, what):
    """sctc_word_lm_score_batch on device labels: (sums float64 [N], counts int32 [N, 2], status int32 [N], terms
    float32 [slots] or None, word ids int32 [slots] or None), device tensors"""
    torch = _sctc.require_gpu()
    N = int(U_b.shape[0])
    lm = lexicon.lm
    flags = (_sctc.WORD_LM_EOS if eos else 0) | (0 if final_word else _sctc.WORD_LM_NO_FINAL_WORD)
    cfg = _sctc.WordLmScoreConfig(N, int(lexicon.A), lexicon.handle, -1 if lm.unk is None else int(lm.unk),
                                  -1 if lm.end is None else int(lm.end), flags, 0, _sctc.i32(U_b), _sctc.i64(loff))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_word_lm_score_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), what)
    device = labels_dev.device
    slots = _sctc.word_lm_slots(U_b)[1]
    sums = torch.empty(N, dtype=torch.float64, device=device)
    counts = torch.empty((N, 2), dtype=torch.int32, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)
    terms = torch.zeros(max(1, slots), dtype=torch.float32, device=device) if want_terms else None
    wids = torch.full((max(1, slots),), -1, dtype=torch.int32, device=device) if want_words else None
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=device)
    rc = L.sctc_word_lm_score_batch(ctypes.byref(cfg), labels_dev.data_ptr(), terms.data_ptr() if want_terms else None,
                                    wids.data_ptr() if want_words else None, sums.data_ptr(), counts.data_ptr(),
                                    status.data_ptr(), ws.data_ptr(), nbytes.value, _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    return sums, counts, status, terms, wids


def word_lm_score_batch(seqs, lexicon, terms=False, words=False, eos=False, final_word=True, device=False):
    """(sums float64 [N], counts int32 [N, 2], status int32 [N]) of label rows under the word LM of ``lexicon`` (a
    :class:`DecodeLexicon`, bigram or n-gram), in one launch on the device: what
    :func:`word_lm_sentence_scores` returns, bit for bit -- its docstring has the rules.  The terms are NATURAL-log
    values, the float32 numbers that :func:`decode_lexicon_beam_batch` adds at the space after a word.

    ``seqs`` as for :func:`lm_score_batch`: a list of CTC symbol-id sequences, or a device triple (ids int32 tensor,
    U, offsets) read in place.  ``terms=True`` / ``words=True`` append the float32 term and the word id (``unk`` for
    an OOV word, ``end`` at the ``</s>`` term) of every word: lists of arrays (empty for a row whose status is not 0),
    or with ``device=True`` flat tensors in which sequence n starts at slot ``sum((U[:n] + 1) // 2 + 1)``.
    ``device=True``: nothing is read back."""
    what = "word_lm_score_batch"
    _word_lexicon(lexicon, what)
    if eos and lexicon.lm.end is None:
        raise ValueError("%s: the LM has no </s>" % what)
    labels, U_b, loff = _score_seqs(seqs, what, _sctc.WORD_LM_MAX_U)
    sums, counts, status, tv, wv = _word_lm_launch(lexicon, labels, U_b, loff, bool(terms), bool(words), eos,
                                                   final_word, what)
    extra = [v for v, want in ((tv, terms), (wv, words)) if want]
    if device:
        return (sums, counts, status) + tuple(extra)
    sums, counts, status = sums.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
    first = _sctc.word_lm_slots(U_b)[0]
    n_terms = np.where(status == 0, counts[:, 0] + (1 if eos else 0), 0)
    lists = []
    for v in extra:
        flat = v.cpu().numpy()
        lists.append([flat[first[n]:first[n] + n_terms[n]].copy() for n in range(U_b.shape[0])])
    return (sums, counts, status) + tuple(lists)


def word_lm_perplexity(sentences_as_label_rows, lexicon, eos=True):
    """(perplexity, n_terms, n_oov) of sentences given as rows of CTC symbols under the word LM of ``lexicon``:
    ``e ** (-sum of the natural-log terms / n_terms)``, n_terms the words plus, with ``eos``, one ``</s>`` a
    sentence; n_oov the words scored as ``<UNK>``.  One :func:`word_lm_score_batch` call.  ValueError for a row the
    LM cannot score, and when there is nothing to score."""
    what = "word_lm_perplexity"
    rows = [np.asarray(s).reshape(-1) for s in sentences_as_label_rows]
    sums, counts, status = word_lm_score_batch(rows, lexicon, eos=eos)
    if (status != 0).any():
        raise ValueError("%s: sentence %d cannot be scored (status %d)"
                         % (what, int(np.nonzero(status)[0][0]), int(status[np.nonzero(status)[0][0]])))
    n = int(counts[:, 0].sum()) + (len(rows) if eos else 0)
    if n == 0:
        raise ValueError("%s: nothing to score" % what)
    return float(np.exp(-float(sums.sum()) / n)), n, int(counts[:, 1].sum())


def rescore_nbest(logprobs, hyps, lengths=None, lm=None, alpha=1.0, beta=0.0, device=False, scores=None, K_b=None,
                  word_lm=None, word_alpha=1.0, word_beta=0.0, word_eos=False, word_final=True):
    """Second pass over n-best lists: every hypothesis gets the score that
    :func:`score_sentences` gives it, log P_ctc(l) + alpha * sum_i log10 P_LM(l_i | <s>, l_<i) + beta * U with the
    full CTC sum, and every utterance's hypotheses are ranked by it -- one forced-alignment launch, one LM-score
    call and one rank launch for the whole batch.  ``lm=None`` ranks by log P_ctc(l) + beta * U.

    logprobs / lengths: as for :func:`decode_beam_batch`.  hyps: the list of lists that
    ``decode_beam_batch(..., nbest=K)`` returns, or the device tensors ``(ids, lens, scores)`` of
    ``decode_beam_batch(..., device=True)``, used in place (only ``lens`` is read back).  The ranks beyond the
    beam (first-pass score -inf) are no hypotheses: they are recognised by the first-pass ``scores`` ([B, K]; the
    device route has them) or by ``K_b`` (int [B]: the leading ranks that are real), stay last and score -inf.
    Returns (order int32 [B, K]: hypothesis indices by descending score, ties to the lower first-pass rank;
    rescored float64 [B, K]: by first-pass rank, -inf where the hypothesis cannot be aligned); device tensors
    with ``device=True``.

    word_lm (a :class:`DecodeLexicon`): one :func:`word_lm_score_batch` launch more over the same labels, and the
    score becomes ``((log P_ctc + alpha * lm) + beta * U) + (word_alpha * word_sum + word_beta * words)`` -- the
    character LM finds the hypotheses, the word LM orders them.  ``word_alpha`` weighs NATURAL-log
    terms (the word LM's unit, as ``alpha`` of :func:`decode_lexicon_beam_batch`); ``alpha`` weighs log10 terms.
    ``word_eos`` / ``word_final`` as ``eos`` / ``final_word`` there.  A hypothesis the word LM cannot score (an OOV
    word under an LM without ``<UNK>``) is -inf."""
    what = "rescore_nbest"
    arrs, src, A, T_b, dt, dtype = _decode_inputs(logprobs, lengths, what)
    B = len(T_b)
    torch = _sctc.require_gpu()
    if lm is not None:
        _lm_kind(lm, what)
        if lm.sym_words.shape[0] < A:
            raise ValueError("%s: the LM maps %d symbols, the input has %d" % (what, lm.sym_words.shape[0], A))
    if word_lm is not None:
        _word_lexicon(word_lm, what)
        if word_lm.A != A:
            raise ValueError("%s: the lexicon was built for %d symbols, the input has %d" % (what, word_lm.A, A))
    Tb = np.ascontiguousarray(T_b, dtype=np.int32)
    foff = np.concatenate([[0], np.cumsum(Tb)[:-1]]).astype(np.int64) if B else np.zeros(0, np.int64)
    first = None
    if isinstance(hyps, tuple) and len(hyps) == 3 and isinstance(hyps[0], torch.Tensor):
        ids, lens, first = hyps
        if lens.numel() % max(B, 1):
            raise ValueError("%s: %d lengths for %d utterances" % (what, lens.numel(), B))
        K = lens.numel() // max(B, 1)
        U_b = np.ascontiguousarray(lens.cpu().numpy(), dtype=np.int32).reshape(-1)
        loff = (K * foff[:, None] + np.arange(K, dtype=np.int64)[None, :] * Tb[:, None].astype(np.int64)).reshape(-1)
        labels = ids
        if U_b.size and int((loff + U_b).max()) > ids.shape[0]:
            raise ValueError("%s: a hypothesis lies outside the ids tensor" % what)
        first = first.reshape(-1).contiguous()
    else:
        if len(hyps) != B:
            raise ValueError("%s: %d n-best lists for %d utterances" % (what, len(hyps), B))
        K = len(hyps[0]) if B else 1
        if any(len(row) != K for row in hyps):
            raise ValueError("%s: every utterance must have the same number of hypotheses" % what)
        labels, U_b, loff = _score_seqs([h for row in hyps for h in row], what, _sctc.ALIGN_MAX_U)
        if scores is not None:
            first = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)).cuda()
            if first.numel() != B * K:
                raise ValueError("%s: scores must be [B, K]" % what)
    if not 1 <= K <= _sctc.NBEST_MAX_K:
        raise ValueError("%s: %d hypotheses per utterance outside 1..%d" % (what, K, _sctc.NBEST_MAX_K))
    if U_b.size and int(U_b.max()) > _sctc.ALIGN_MAX_U:
        raise ValueError("%s: a hypothesis of %d labels, the limit is %d" % (what, int(U_b.max()), _sctc.ALIGN_MAX_U))
    loff = np.ascontiguousarray(loff, dtype=np.int64)
    Kb = np.full(B, K, dtype=np.int32) if K_b is None else np.ascontiguousarray(K_b, dtype=np.int32).reshape(-1)
    if Kb.shape[0] != B:
        raise ValueError("%s: K_b must be [B]" % what)
    # ---- one forced-alignment launch over the B * K pairs: the K hypotheses of an utterance share its frames ----
    ld = int(A)
    if src is not None:
        dev = src if src.stride(1) == 1 and A <= src.stride(0) < 2 ** 31 else src.contiguous()
        ld = int(dev.stride(0))
    else:
        host = np.concatenate([np.ascontiguousarray(p.T, dtype=dt) for p in arrs], axis=0) if sum(T_b) else \
            np.zeros((1, A), dtype=dt)
        dev = torch.from_numpy(host).cuda()
    labels = labels.to(dev.device)
    P = B * K
    T_p = np.ascontiguousarray(np.repeat(Tb, K), dtype=np.int32)
    f_p = np.ascontiguousarray(np.repeat(foff, K), dtype=np.int64)
    cfg = _sctc.AlignConfig(P, int(A), dtype, 0, ld, _sctc.ALIGN_TOTAL, _sctc.i32(T_p), _sctc.i64(f_p), _sctc.i32(U_b),
                            _sctc.i64(loff))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_ctc_align_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), what)
    device_ = dev.device
    a_scores = torch.empty((max(P, 1), 2), dtype=torch.float64, device=device_)
    a_status = torch.empty(max(P, 1), dtype=torch.int32, device=device_)
    # the alignments themselves are not wanted; hypotheses of one utterance write the same frame labels
    junk = torch.empty(int(Tb.sum()) + 2 * int(U_b.sum()) + 2, dtype=torch.int32, device=device_)
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=device_)
    rc = L.sctc_ctc_align_batch(ctypes.byref(cfg), dev.data_ptr(), labels.data_ptr(), junk.data_ptr(),
                                junk.data_ptr() + 4 * int(Tb.sum()), a_scores.data_ptr(), a_status.data_ptr(),
                                ws.data_ptr() if nbytes.value else None, nbytes.value, _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    # ---- one LM-score call ----
    lm_sums = None
    if lm is not None and P:
        lm_sums, _, _ = _lm_score_launch(lm, lm.sym_words[:A], labels, U_b, loff, False, what)
    # ---- one rank launch ----
    rescored = torch.empty((B, K), dtype=torch.float64, device=device_)
    order = torch.empty((B, K), dtype=torch.int32, device=device_)
    head = (B, K, _sctc.i32(Kb), _sctc.i32(U_b), float(alpha), float(beta), a_scores.data_ptr(), a_status.data_ptr(),
            lm_sums.data_ptr() if lm_sums is not None else None, first.data_ptr() if first is not None else None)
    tail = (rescored.data_ptr(), order.data_ptr(), _sctc.current_stream_ptr())
    if word_lm is not None and P:
        # ---- one word-LM call, and the rank entry that takes its sums ----
        w_sums, w_counts, w_status, _, _ = _word_lm_launch(word_lm, labels, U_b, loff, False, False, word_eos,
                                                           word_final, what)
        rc = L.sctc_nbest_rank_words_batch(*(head + (w_sums.data_ptr(), w_counts.data_ptr(), w_status.data_ptr(),
                                                     float(word_alpha), float(word_beta)) + tail))
    else:
        rc = L.sctc_nbest_rank_batch(*(head + tail))
    _sctc.check(rc, what)
    if device:
        return order, rescored
    return order.cpu().numpy(), rescored.cpu().numpy()


def nbest_oracle(refs, nbest_hyps):
    """Oracle error of n-best lists: for utterance b the hypothesis of ``nbest_hyps[b]`` (the list
    that ``decode_beam_batch(..., nbest=k)`` returns for it) closest to ``refs[b]``.  An empty
    hypothesis is a hypothesis like any other; a caller that wants the ranks beyond the beam
    (empty, score -inf) left out drops them first.  Returns ``(best_index, best_dist,
    first_dist)``, int32 [B] each: the rank of the closest hypothesis (ties: the lowest rank),
    its distance, and the distance of rank 0; -1 / -1 / -1 for an utterance without hypotheses.
    One :func:`edit_distance_batch` call; every reference is uploaded once."""
    B = len(refs)
    if len(nbest_hyps) != B:
        raise ValueError("nbest_oracle: %d references for %d n-best lists" % (B, len(nbest_hyps)))
    hyps, a_index, count = [], [], []
    for b, row in enumerate(nbest_hyps):
        row = list(row)
        hyps.extend(row)
        a_index.extend([b] * len(row))
        count.append(len(row))
    stats = edit_distance_batch(refs, hyps, a_index=a_index)
    best_index = np.full(B, -1, dtype=np.int32)
    best_dist = np.full(B, -1, dtype=np.int32)
    first_dist = np.full(B, -1, dtype=np.int32)
    o = 0
    for b in range(B):
        if count[b]:
            d = stats[o:o + count[b], 0]
            best_index[b] = int(np.argmin(d))      # the first minimum
            best_dist[b] = d[best_index[b]]
            first_dist[b] = d[0]
        o += count[b]
    return best_index, best_dist, first_dist


# ---- word interning, minimum Bayes risk selection and word confidences over n-best lists ----

def _alphabet_space(A, space, what, need_space=True):
    A = int(A)
    if not 1 <= A <= 256:
        raise ValueError("%s: alphabet of %d symbols outside 1..256" % (what, A))
    if need_space:
        if space is None or not 1 <= int(space) < A:
            raise ValueError("%s: the space symbol must lie in [1, %d)" % (what, A))
    return A, 1 if space is None else int(space)


def _intern_launch(labels_dev, U_b, loff, goff, A, space, what):
    """sctc_intern_words_batch on device labels: (word ids int32 [slots] with -1 in the slots that hold no word,
    counts int32 [N], status int32 [N]), device tensors"""
    torch = _sctc.require_gpu()
    N = int(U_b.shape[0])
    goff = np.ascontiguousarray(goff, dtype=np.int32)
    cfg = _sctc.InternConfig(N, int(goff.shape[0]) - 1, A, space, _sctc.i32(U_b), _sctc.i64(loff), _sctc.i32(goff))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_intern_words_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), what)
    device = labels_dev.device
    slots = _sctc.intern_slots(U_b)[1]
    ids = torch.full((max(1, slots),), -1, dtype=torch.int32, device=device)
    counts = torch.empty(max(1, N), dtype=torch.int32, device=device)[:N]
    status = torch.empty(max(1, N), dtype=torch.int32, device=device)[:N]
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=device)
    rc = L.sctc_intern_words_batch(ctypes.byref(cfg), labels_dev.data_ptr(), ids.data_ptr(), counts.data_ptr(),
                                   status.data_ptr(), ws.data_ptr(), nbytes.value, _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    return ids, counts, status


def _group_offsets(groups, N, what):
    goff = np.asarray(groups, dtype=np.int64).reshape(-1)
    if goff.shape[0] < 1 or goff[0] != 0 or goff[-1] != N or (np.diff(goff) < 0).any():
        raise ValueError("%s: groups must be row offsets that run from 0 to %d and never decrease" % (what, N))
    return goff.astype(np.int32)


def intern_words(seqs, groups, space, A=256, device=False):
    """Word ids of label rows without a lexicon: a word is a maximal run of symbols other than
    ``space`` (``str.split()``), and within a group of rows two words get the same id exactly when they are the same
    run of symbols -- the id is the number, in (row, position) order within the group, of the word's first
    occurrence.  Distinct out-of-vocabulary words therefore stay distinct, which the lexicon's ids do not offer.

    ``seqs`` as for :func:`lm_score_batch`: a list of CTC symbol-id rows (at most 4095 symbols), or a device triple
    (ids int32 tensor, U, offsets) read in place.  ``groups``: the G + 1 row offsets of G groups of consecutive rows,
    from 0 to the number of rows.  Returns (ids, counts): a list of int32 arrays, one per row, and int32 [N]; a row
    with a symbol outside [1, A) is a ValueError.  ``device=True``: nothing is read back; ids is one flat int32
    tensor in which row n starts at slot ``sum((U[:n] + 1) // 2)`` (slots past a row's words hold -1), counts a
    device tensor, and a row with a symbol outside [1, A) has count 0."""
    what = "intern_words"
    A, space = _alphabet_space(A, space, what)
    labels, U_b, loff = _score_seqs(seqs, what, _sctc.MBR_MAX_U)
    goff = _group_offsets(groups, U_b.shape[0], what)
    ids, counts, status = _intern_launch(labels, U_b, loff, goff, A, space, what)
    if device:
        return ids, counts
    flat, counts, status = ids.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
    if (status != 0).any():
        raise ValueError("%s: row %d has a symbol outside [1, %d)" % (what, int(np.nonzero(status)[0][0]), A))
    first = _sctc.intern_slots(U_b)[0]
    return [flat[first[n]:first[n] + counts[n]].copy() for n in range(U_b.shape[0])], counts


def word_errors_batch(refs, hyps, space, A=256):
    """int32 [P, 5]: the columns of :func:`edit_distance_batch` (distance, UP, LEFT, SUB, MATCH with a = ref,
    b = hyp) counted in WORDS, for P pairs of CTC symbol rows -- what ``editDistance.edit_distance(ref.split(),
    hyp.split())`` returns.  Every {reference, hypothesis} pair is interned as a group on the device
    (:func:`intern_words`), the counts come back in one small read-back, and :func:`edit_distance_device` runs on
    the ids in place."""
    what = "word_errors_batch"
    A, space = _alphabet_space(A, space, what)
    refs, hyps = list(refs), list(hyps)
    P = len(refs)
    if len(hyps) != P:
        raise ValueError("%s: %d references for %d hypotheses" % (what, P, len(hyps)))
    if P == 0:
        return np.zeros((0, 5), dtype=np.int32)
    rows = [r for pair in zip(refs, hyps) for r in pair]
    labels, U_b, loff = _score_seqs(rows, what, _sctc.MBR_MAX_U)
    torch = _sctc.require_gpu()
    ids, counts, status = _intern_launch(labels, U_b, loff, 2 * np.arange(P + 1), A, space, what)
    back = torch.stack([counts, status]).cpu().numpy()
    if (back[1] != 0).any():
        raise ValueError("%s: row %d has a symbol outside [1, %d)" % (what, int(np.nonzero(back[1])[0][0]), A))
    first = _sctc.intern_slots(U_b)[0]
    stats = edit_distance_device(ids, back[0][0::2], first[0::2], ids, back[0][1::2], first[1::2])
    return stats.cpu().numpy()


def mbr_nbest(hyps, scores, unit="word", scale=1.0, space=None, order=None, K_b=None, confidences=False,
              distances=False, device=False, A=256, lengths=None):
    """Minimum Bayes risk selection over n-best lists on the device: with posteriors
    ``p_k = w_k / Z``, ``w_k = exp(scale * (s_k - s_max))`` over the real hypotheses of an utterance, the chosen
    hypothesis is the one of least expected edit distance ``risk_k = sum_j p_j D(k, j)`` to the others, D counted
    in symbols (``unit="char"``) or in words (``unit="word"``, the words interned per utterance as
    :func:`intern_words` does; ``space`` is then required).

    hyps: the list of lists that ``decode_beam_batch(..., nbest=K)`` returns, or the device tensors
    ``(ids, lens, scores)`` of ``decode_beam_batch(..., device=True)`` used in place, with ``lengths`` the frames
    T_b of the utterances (they fix where the ranks lie in ``ids``).  scores: [B, K], array or device tensor --
    ``rescored`` of :func:`rescore_nbest` or the first pass's; a hypothesis whose score is not finite, or whose rank
    is not below ``K_b[b]``, is not real.  order: the ``order`` of :func:`rescore_nbest` ([B, K]) or None; risk
    ties go to the hypothesis that comes first in it, without it to the lower rank.

    Returns a dict: ``best`` int32 [B] (-1 without a real hypothesis), ``posterior`` and ``risk`` float64 [B, K]
    (0 and +inf for a rank that is not real), ``order`` int32 [B, K] (ranks by ascending risk, the ranks that are
    not real last); with ``distances`` also ``dist`` int32 [B, K, K] (-1 for a rank that is not real); with
    ``confidences`` also ``confidence``, a list of float64 arrays: for every unit of the chosen hypothesis the
    posterior mass of the hypotheses whose alignment with it (the path of :func:`edit_distance_batch`) has a MATCH
    there.  ``device=True``: nothing is read back, the values are device tensors and ``confidence`` is the pair
    (flat float64 tensor, in which utterance b starts at the sum of the earlier utterances' longest unit bounds --
    U in character unit, ceil(U / 2) in word unit, over the ranks below K_b -- and ``conf_len`` int32 [B])."""
    what = "mbr_nbest"
    if unit not in ("char", "word"):
        raise ValueError("%s: unit must be 'char' or 'word'" % what)
    words = unit == "word"
    A, space = _alphabet_space(A, space, what, need_space=words)
    scale = float(scale)
    if not np.isfinite(scale) or scale < 0:
        raise ValueError("%s: scale must be a finite number >= 0" % what)
    torch = _sctc.require_gpu()
    if isinstance(hyps, tuple) and len(hyps) == 3 and isinstance(hyps[0], torch.Tensor):
        if lengths is None:
            raise ValueError("%s: the device tensors of a search need lengths" % what)
        ids, lens, _ = hyps
        Tb = np.ascontiguousarray([int(t) for t in lengths], dtype=np.int64)
        B = Tb.shape[0]
        if lens.numel() % max(B, 1):
            raise ValueError("%s: %d lengths for %d utterances" % (what, lens.numel(), B))
        K = lens.numel() // max(B, 1)
        foff = np.concatenate([[0], np.cumsum(Tb)[:-1]]).astype(np.int64) if B else np.zeros(0, np.int64)
        loff = (K * foff[:, None] + np.arange(K, dtype=np.int64)[None, :] * Tb[:, None]).reshape(-1)
        labels, U_b, loff = _score_seqs((ids, lens, loff), what, _sctc.MBR_MAX_U)
    else:
        B = len(hyps)
        K = len(hyps[0]) if B else 1
        if any(len(row) != K for row in hyps):
            raise ValueError("%s: every utterance must have the same number of hypotheses" % what)
        labels, U_b, loff = _score_seqs([h for row in hyps for h in row], what, _sctc.MBR_MAX_U)
    if not 1 <= K <= _sctc.NBEST_MAX_K:
        raise ValueError("%s: %d hypotheses per utterance outside 1..%d" % (what, K, _sctc.NBEST_MAX_K))
    device_ = labels.device
    if isinstance(scores, torch.Tensor):
        sc = scores.to(device=device_, dtype=torch.float64).reshape(-1).contiguous()
    else:
        sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)).to(device_)
    if sc.numel() != B * K:
        raise ValueError("%s: scores must be [B, K]" % what)
    od = None
    if order is not None:
        if isinstance(order, torch.Tensor):
            od = order.to(device=device_, dtype=torch.int32).reshape(-1).contiguous()
        else:
            od = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32).reshape(-1)).to(device_)
        if od.numel() != B * K:
            raise ValueError("%s: order must be [B, K]" % what)
    Kb = np.full(B, K, dtype=np.int32) if K_b is None else np.ascontiguousarray(K_b, dtype=np.int32).reshape(-1)
    if Kb.shape[0] != B or (B and (Kb.min() < 0 or Kb.max() > K)):
        raise ValueError("%s: K_b must be [B] with entries in 0..%d" % (what, K))
    loff = np.ascontiguousarray(loff, dtype=np.int64)
    flags = (_sctc.MBR_CONF if confidences else 0) | (_sctc.MBR_DIST if distances else 0)
    cfg = _sctc.MbrConfig(B, K, _sctc.MBR_WORDS if words else _sctc.MBR_CHARS, flags, A, space, scale, _sctc.i32(Kb),
                          _sctc.i32(U_b), _sctc.i64(loff))
    L = _sctc.lib()
    nbytes = ctypes.c_size_t(0)
    _sctc.check(L.sctc_nbest_mbr_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)), what)
    post = torch.empty((B, K), dtype=torch.float64, device=device_)
    risk = torch.empty((B, K), dtype=torch.float64, device=device_)
    best = torch.empty(B, dtype=torch.int32, device=device_)
    m_order = torch.empty((B, K), dtype=torch.int32, device=device_)
    dist = torch.empty((B, K, K), dtype=torch.int32, device=device_) if distances else None
    conf = conf_len = None
    if confidences:
        bound = ((U_b.astype(np.int64) + 1) // 2 if words else U_b.astype(np.int64)).reshape(B, K)
        bound = np.where(np.arange(K)[None, :] < Kb[:, None], bound, 0)
        conf_first = np.concatenate([[0], np.cumsum(bound.max(axis=1) if B else [])]).astype(np.int64)
        conf = torch.zeros(max(1, int(conf_first[-1])), dtype=torch.float64, device=device_)
        conf_len = torch.zeros(max(1, B), dtype=torch.int32, device=device_)[:B]
    ws = torch.empty(max(1, nbytes.value), dtype=torch.uint8, device=device_)
    rc = L.sctc_nbest_mbr_batch(ctypes.byref(cfg), labels.data_ptr(), sc.data_ptr(), od.data_ptr() if od is not None else None,
                                post.data_ptr(), risk.data_ptr(), best.data_ptr(), m_order.data_ptr(),
                                dist.data_ptr() if distances else None, conf.data_ptr() if confidences else None,
                                conf_len.data_ptr() if confidences else None, ws.data_ptr(), nbytes.value,
                                _sctc.current_stream_ptr())
    _sctc.check(rc, what)
    out = {"best": best, "posterior": post, "risk": risk, "order": m_order}
    if distances:
        out["dist"] = dist
    if device:
        if confidences:
            out["confidence"] = (conf, conf_len)
        return out
    out = {k: v.cpu().numpy() for k, v in out.items()}
    if confidences:
        flat, n = conf.cpu().numpy(), conf_len.cpu().numpy()
        out["confidence"] = [flat[conf_first[b]:conf_first[b] + n[b]].copy() for b in range(B)]
    return out
