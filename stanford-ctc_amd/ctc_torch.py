"""The CTC kernels of libsctc_hip.so as a differentiable PyTorch loss on time-major ``[T, N, C]`` tensors: a
drop-in for ``torch.nn.functional.ctc_loss`` / ``torch.nn.CTCLoss`` on the MI355X.

    ctc_loss(input, targets, input_lengths, target_lengths, blank=0, reduction="mean",
             zero_infinity=False, logits=False) -> tensor
    CTCLoss(blank=0, reduction="mean", zero_infinity=False, logits=False)      # nn.Module, called like torch.nn.CTCLoss

``input`` is a CUDA tensor ``[T, N, C]``, float32 or float64, of ANY strides (an ``[N, T, C]`` tensor seen through
``.transpose(0, 1)`` is read in place; no ``.contiguous()`` copy is made).  It holds log-probabilities, as for
``torch.nn.functional.ctc_loss``; with ``logits=True`` it holds unnormalised activations and the softmax is computed
by the prologue kernel.  ``targets`` is an integer tensor, ``[N, S]`` padded or 1-D concatenated, on the CPU or on the
device; entries beyond ``target_lengths[n]`` are never read or validated (padding of -1 or of values >= C is legal).
``input_lengths`` and ``target_lengths`` are tensors, lists or tuples.

Labels and lengths go to the HOST, because ``sctc_ctc_loss_batch`` takes host arrays: when they live on the device,
that is one device-to-host copy (a synchronisation) per such tensor and call.  Keep them on the CPU to avoid it.

The returned gradient.  In both modes the gradient with respect to ``input`` is ``p - occupancy``, p the (softmax)
probabilities: the reference's ``grad`` (ctc_fast.pyx:138-145), the derivative with respect to the activations IN FRONT
of the softmax.  For ``logits=True`` that is the derivative with respect to ``input`` itself.  For log-probabilities
it is what PyTorch's native backward returns as well: PyTorch, too, assumes a ``log_softmax`` upstream, through which
the ``p`` term vanishes.  So ``torch.autograd.gradcheck`` is meaningful on ``logits=True`` and on the composition
``log_softmax`` -> ``logits=False``, not on raw log-probabilities alone -- as with ``torch.nn.functional.ctc_loss``.

Semantics are PyTorch's: ``reduction`` "none" gives the ``[N]`` losses, "sum" their sum, "mean" each loss divided by
``max(target_length, 1)`` and then the batch mean; an empty target costs ``-sum_t log p[t, n, blank]``; the gradient of
the padded frames ``t >= input_lengths[n]`` is exactly 0.  An infeasible utterance (cost +inf, or the reference's
``skip``: a frame normaliser of 0) has loss ``+inf``, or 0 with ``zero_infinity=True``.  The ONE deliberate
difference: the gradient of such an utterance is ALWAYS exact zeros (PyTorch gives NaN there without
``zero_infinity``; the reference drops the utterance from the update).

One frame (``input_lengths[n] == 1``) is the one shape where the reference's cost is not the CTC loss (it returns
``-log(p_blank + p_label)``, ctc_fast.pyx:42-47, and the CTC kernels follow it); such utterances are answered as PyTorch
answers them, ``-log p_label`` for one label and ``+inf`` for more, outside the CTC call.

fp16 / bf16 inputs raise ``TypeError`` (call ``.float()``); there is no double backward.  Argument errors are raised
before the GPU is touched.  There is no CPU fallback: a CPU ``input`` raises.

The same module holds minimum word error rate training over n-best lists, on the same kernels:

    mwer_loss(input, hyps, hyp_lengths, errors, input_lengths, hyp_counts=None, blank=0, scale=1.0,
              reduction="mean", subtract_mean=True, logits=False, return_stats=False)
    MWERLoss(blank=0, scale=1.0, reduction="mean", subtract_mean=True, logits=False)     # nn.Module
    mwer_nbest(input, input_lengths, references, reference_lengths, nbest, beam=40, unit="word", space=None,
               lm=None, alpha=1.0, beta=0.0, logits=False)

whose semantics stand in the docstring of :func:`mwer_loss`.
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

import _sctc

_REDUCTIONS = ("none", "mean", "sum")


# ---------------------------------------------------------------- host helpers (no GPU: tests/test_ctc_torch_cpu.py)

def _host_lengths(x, N, what):
    """a tensor, list or tuple of N integers -> int64 NumPy vector on the host"""
    if isinstance(x, torch.Tensor):
        if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
            raise TypeError("ctc_loss: %s must hold integers, not %s" % (what, x.dtype))
        x = x.detach().cpu().numpy()
    arr = np.asarray(x)
    if arr.size and arr.dtype.kind not in "iu":
        raise TypeError("ctc_loss: %s must hold integers" % what)
    if arr.ndim != 1 or arr.shape[0] != N:
        raise ValueError("ctc_loss: %s must have one entry per utterance (%d), got shape %s" % (what, N, tuple(arr.shape)))
    return arr.astype(np.int64)


def _host_targets(targets, target_lengths, N, C):
    """targets ([N, S] padded or 1-D concatenated, any integer dtype, any device) -> (labels, U, off): the labels of
    all utterances concatenated (int32), labels per utterance (int32 [N]) and the first label of each (int64 [N]).
    Only the first target_lengths[n] entries of a row are read."""
    if not isinstance(targets, torch.Tensor):
        raise TypeError("ctc_loss: targets must be a tensor")
    if targets.is_floating_point() or targets.is_complex() or targets.dtype == torch.bool:
        raise TypeError("ctc_loss: targets must hold integers, not %s" % targets.dtype)
    U = _host_lengths(target_lengths, N, "target_lengths")
    tg = targets.detach().cpu().numpy()
    if tg.ndim == 2:
        if tg.shape[0] != N:
            raise ValueError("ctc_loss: targets has %d rows for %d utterances" % (tg.shape[0], N))
        S = tg.shape[1]
        if U.size and (U.min() < 0 or U.max() > S):
            raise ValueError("ctc_loss: target_lengths must lie in [0, %d]" % S)
        parts = [tg[n, :U[n]] for n in range(N)]
        labels = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    elif tg.ndim == 1:
        if U.size and U.min() < 0:
            raise ValueError("ctc_loss: negative target length")
        if int(U.sum()) > tg.shape[0]:
            raise ValueError("ctc_loss: %d concatenated targets for target_lengths that sum to %d" % (tg.shape[0], U.sum()))
        labels = tg[:int(U.sum())]
    else:
        raise ValueError("ctc_loss: targets must be [N, S] or 1-D, got %d dimensions" % tg.ndim)
    if labels.size and (labels.min() < 0 or labels.max() >= C):
        raise ValueError("ctc_loss: a target label lies outside [0, %d)" % C)
    off = np.zeros(N, dtype=np.int64)
    if N > 1:
        off[1:] = np.cumsum(U)[:-1]
    return np.ascontiguousarray(labels, dtype=np.int32), U.astype(np.int32), off


def _reduce(losses, target_lengths, reduction):
    """PyTorch's reduction of the [N] losses; target_lengths a tensor on the losses' device"""
    if reduction == "none":
        return losses
    if reduction == "sum":
        return losses.sum()
    return (losses / target_lengths.clamp(min=1).to(losses.dtype)).mean()


def _scale(grad_output, target_lengths, reduction, N):
    """d (reduced loss) / d losses[n], times grad_output, as float64 [N]: the factor of utterance n's gradient rows"""
    go = grad_output.to(torch.float64)
    if reduction == "none":
        return go.reshape(N)
    if reduction == "sum":
        return go.reshape(()).expand(N)
    return go.reshape(()) / (target_lengths.clamp(min=1).to(torch.float64) * N)


def _check_args(input, targets, input_lengths, target_lengths, blank, reduction):
    """every argument error, on the host; returns (T_n, labels, U, off)"""
    if not isinstance(input, torch.Tensor):
        raise TypeError("ctc_loss: input must be a tensor")
    if input.dtype in (torch.float16, torch.bfloat16):
        raise TypeError("ctc_loss: %s input is not supported: call .float() on it" % input.dtype)
    if input.dtype not in (torch.float32, torch.float64):
        raise TypeError("ctc_loss: input must be float32 or float64, not %s" % input.dtype)
    if input.dim() != 3:
        raise ValueError("ctc_loss: input must be [T, N, C], got %d dimensions" % input.dim())
    if reduction not in _REDUCTIONS:
        raise ValueError("ctc_loss: %r is not a reduction (none, mean, sum)" % (reduction,))
    T, N, C = input.shape
    if C < 1:
        raise ValueError("ctc_loss: empty alphabet")
    if not 0 <= int(blank) < C:
        raise ValueError("ctc_loss: blank %d outside [0, %d)" % (blank, C))
    if T * N > 2 ** 31 - 1:
        raise ValueError("ctc_loss: T * N = %d rows do not fit the kernels' int32 row index" % (T * N))
    T_n = _host_lengths(input_lengths, N, "input_lengths")
    if T_n.size and (T_n.min() < 1 or T_n.max() > T):
        raise ValueError("ctc_loss: input_lengths must lie in [1, %d]" % T)
    labels, U, off = _host_targets(targets, target_lengths, N, C)
    return T_n.astype(np.int32), labels, U, off


# ---------------------------------------------------------------- the autograd function

def _cfg(x, mode, blank):
    T, N, C = x.shape
    st, sn, sc = x.stride()
    return _sctc.TncConfig(T, N, C, _sctc.F64 if x.dtype == torch.float64 else _sctc.F32, mode, blank, st, sn, sc)


class _CtcLossTnc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, host, blank, reduction, zero_infinity, logits):
        T_n, labels, U, off = host
        T, N, C = input.shape
        dev = input.device
        L = _sctc.lib()
        with torch.cuda.device(dev):
            stream = _sctc.current_stream_ptr()
            T_dev = torch.from_numpy(T_n).to(dev)
            U_dev = torch.from_numpy(U).to(dev)
            probs = torch.empty((T * N, C), dtype=input.dtype, device=dev)
            grad = torch.empty_like(probs)
            cost = torch.empty(N, dtype=torch.float64, device=dev)
            skip = torch.empty(N, dtype=torch.int32, device=dev)
            cfg = _cfg(input, _sctc.TNC_LOGITS if logits else _sctc.TNC_LOG_PROBS, blank)
            _sctc.check(L.sctc_ctc_tnc_probs(ctypes.byref(cfg), input.data_ptr(), T_dev.data_ptr(), probs.data_ptr(),
                                             stream), "ctc_tnc_probs")
            # Utterances with ONE alignment that emits one symbol in every frame go to the empty-target kernel: an
            # empty target (the blank), and one label in one frame (the label) -- there the reference normalises
            # over blank + label before any band applies (ctc_fast.pyx:42-47), and the CTC kernels follow it to
            # -log(p_blank + p_label), where the loss is -log p_label.  For the same reason one frame for two labels or
            # more is answered here: infeasible
            one_frame = (T_n == 1) & (U >= 1)
            single = np.flatnonzero((U == 0) | (one_frame & (U == 1)))
            never = np.flatnonzero(one_frame & (U > 1))
            full = np.flatnonzero((U > 0) & ~one_frame)
            if never.size:
                at = torch.from_numpy(never).to(dev)
                cost[at] = float("inf")
                skip[at] = 1
            if full.size:
                # the [T * N][C] buffer as a batch of the CTC entry: frame t of utterance n is row t * N + n
                rowbase = torch.arange(T, dtype=torch.int32, device=dev) * N
                whole = full.size == N
                cost_b = cost if whole else torch.empty(full.size, dtype=torch.float64, device=dev)
                skip_b = skip if whole else torch.empty(full.size, dtype=torch.int32, device=dev)
                T_b = np.ascontiguousarray(T_n[full])
                U_b = np.ascontiguousarray(U[full])
                f_off = np.ascontiguousarray(full, dtype=np.int64)
                l_off = np.ascontiguousarray(off[full])
                bt = _sctc.CtcBatch(int(full.size), C, blank, cfg.dtype, C, _sctc.i32(T_b), _sctc.i32(U_b),
                                    _sctc.i64(f_off), _sctc.i32(labels), _sctc.i64(l_off),
                                    ctypes.c_void_p(rowbase.data_ptr()))
                nbytes = L.sctc_ctc_workspace_bytes(ctypes.byref(bt))
                if nbytes == 0:
                    _sctc.check(-1, "ctc_loss")
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _sctc.check(L.sctc_ctc_loss_batch(ctypes.byref(bt), probs.data_ptr(), grad.data_ptr(), cost_b.data_ptr(),
                                                  skip_b.data_ptr(), ws.data_ptr(), nbytes, stream), "ctc_loss")
                if not whole:
                    at = torch.from_numpy(f_off).to(dev)
                    cost[at] = cost_b
                    skip[at] = skip_b
            if single.size:
                sym = np.where(U[single] == 0, blank, labels[np.minimum(off[single], max(labels.size - 1, 0))]
                               if labels.size else blank)
                both = torch.from_numpy(np.ascontiguousarray(np.stack([single, sym]), dtype=np.int32)).to(dev)
                _sctc.check(L.sctc_ctc_tnc_empty(ctypes.byref(cfg), probs.data_ptr(), T_dev.data_ptr(), both[0].data_ptr(),
                                                 both[1].data_ptr(), int(single.size), grad.data_ptr(), cost.data_ptr(),
                                                 skip.data_ptr(), stream), "ctc_tnc_empty")
            infeasible = (skip != 0) | (cost == float("inf"))
            fill = 0.0 if zero_infinity else float("inf")
            losses = torch.where(infeasible, torch.full_like(cost, fill), cost).to(input.dtype)
            if ctx.needs_input_grad[0]:
                ctx.save_for_backward(grad, cost, skip, T_dev, U_dev)
                ctx.meta = (tuple(input.shape), input.dtype, blank, reduction)
            return _reduce(losses, U_dev, reduction)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        grad, cost, skip, T_dev, U_dev = ctx.saved_tensors
        shape, dtype, blank, reduction = ctx.meta
        N = shape[1]
        with torch.cuda.device(grad.device):
            scale = _scale(grad_output, U_dev, reduction, N).contiguous()
            out = torch.empty(shape, dtype=dtype, device=grad.device)
            cfg = _cfg(out, _sctc.TNC_LOG_PROBS, blank)
            _sctc.check(_sctc.lib().sctc_ctc_tnc_grad(ctypes.byref(cfg), grad.data_ptr(), T_dev.data_ptr(),
                                                      cost.data_ptr(), skip.data_ptr(), scale.data_ptr(),
                                                      out.data_ptr(), _sctc.current_stream_ptr()), "ctc_tnc_grad")
        return out, None, None, None, None, None


def ctc_loss(input, targets, input_lengths, target_lengths, blank=0, reduction="mean", zero_infinity=False,
             logits=False):
    """CTC loss of a time-major batch; the arguments and semantics of ``torch.nn.functional.ctc_loss`` plus
    ``logits`` (module docstring).  The gradient with respect to ``input`` is ``p - occupancy`` in both modes."""
    host = _check_args(input, targets, input_lengths, target_lengths, blank, reduction)
    if not input.is_cuda:
        _sctc.require_gpu()
        raise _sctc.SctcError("ctc_loss: input lives on %s: the CTC kernels have no CPU fallback" % input.device)
    return _CtcLossTnc.apply(input, host, int(blank), reduction, bool(zero_infinity), bool(logits))


class CTCLoss(torch.nn.Module):
    """``torch.nn.CTCLoss`` over the CTC kernels of libsctc_hip.so; ``forward(input, targets, input_lengths,
    target_lengths)``.  ``logits=True``: ``input`` holds unnormalised activations (no ``log_softmax`` in front)."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False, logits=False):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError("CTCLoss: %r is not a reduction (none, mean, sum)" % (reduction,))
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity
        self.logits = logits

    def forward(self, input, targets, input_lengths, target_lengths):
        return ctc_loss(input, targets, input_lengths, target_lengths, self.blank, self.reduction, self.zero_infinity,
                        self.logits)


# ================================================================ minimum word error rate training

_MWER_DOC = """Minimum word error rate training over n-best lists (MWER, Prabhavalkar et al. 2018; DESIGN.md §4.16): the
expected number of errors under the model's own posterior over the hypotheses of every utterance.

Utterance n has frames ``T_n`` and hypotheses ``k < K_n[n] <= K`` with label rows ``y_k`` (length ``U_k >= 0``, labels
in ``[0, C)``, none equal to the blank) and errors ``W_k`` (float64, any unit the caller likes).

* ``ll_k = log P_ctc(y_k | x_n)``, float64: minus the cost the CTC kernels return for that label row over that
  utterance's probabilities.
* Real.  Hypothesis k is real when ``k < K_n[n]``, ``W_k`` is finite, the CTC call's ``skip`` is 0 and its cost is
  finite.  Everything else has weight 0 and is never read beyond that test; its labels are not validated.
* Active.  An utterance is active when ``T_n >= 2`` and it has at least one real hypothesis.  An inactive utterance
  has loss 0 and gradient rows of exact zeros.  (One frame is the shape where the CTC kernels follow the reference to
  ``-log(p_blank + p_label)`` instead of the CTC loss; MWER over a one-frame utterance is of no use, so it is left out,
  not special-cased.)
* Weights.  ``m = max ll_k`` over the real ones; ``w_k = exp(scale * (ll_k - m))``; ``Z = sum w_k`` in ascending k;
  ``P_k = w_k / Z``; ``R = sum P_k W_k`` in ascending k, the expected error; ``Wbar = (sum W_k, ascending k) / (number
  of real hypotheses)``.  Everything is float64.
* Loss.  ``loss_n = R - Wbar``, or ``R`` alone with ``subtract_mean=False``.  The baseline changes the value, never
  the gradient.
* Coefficients.  ``c_k = scale * P_k * (W_k - R)``: this is ``d loss_n / d ll_k``.
* Gradient.  ``d loss_n / d input[t, n, c] = sum_k c_k * occ_k[t, c]`` for ``t < T_n``, exact 0 for padded frames;
  ``occ_k = p - g_k`` is the occupancy of symbol c at frame t under hypothesis k, ``p`` the probabilities and ``g_k``
  the gradient row the CTC kernels return.  Because ``sum_k c_k = 0`` the ``p`` term that ``ctc_loss`` carries
  cancels: the sum is the exact derivative both with respect to activations in front of a softmax (``logits=True``)
  and with respect to raw log-probabilities (``logits=False``).  So ``torch.autograd.gradcheck`` is meaningful in BOTH
  modes here, unlike for ``ctc_loss``.
"""

MWER_MAX_K = _sctc.NBEST_MAX_K


def _host_matrix(x, shape, what, integers):
    """a tensor or array-like of `shape` -> NumPy array on the host (int64, or float64)"""
    if isinstance(x, torch.Tensor):
        if x.is_complex() or x.dtype == torch.bool or (integers and x.is_floating_point()):
            raise TypeError("mwer_loss: %s must hold %s, not %s" % (what, "integers" if integers else "real numbers", x.dtype))
        x = x.detach().cpu()
        x = (x if integers else x.to(torch.float64)).numpy()
    arr = np.asarray(x)
    if arr.size and arr.dtype.kind not in ("iu" if integers else "iuf"):
        raise TypeError("mwer_loss: %s must hold %s" % (what, "integers" if integers else "real numbers"))
    if tuple(arr.shape) != tuple(shape):
        raise ValueError("mwer_loss: %s must have shape %s, got %s" % (what, tuple(shape), tuple(arr.shape)))
    return arr.astype(np.int64 if integers else np.float64)


def _mwer_check_args(input, hyps, hyp_lengths, errors, input_lengths, hyp_counts, blank, scale, reduction):
    """every argument error, on the host; returns (T_n, K_n int32 [N], W float64 [N, K], full, empty: bool [N, K],
    labels int32, U int32 [N, K]).  `full` marks the hypotheses that go to the CTC call, `empty` those without labels;
    a slot in neither is never read again: its labels and its length are not validated."""
    if not isinstance(input, torch.Tensor):
        raise TypeError("mwer_loss: input must be a tensor")
    if input.dtype in (torch.float16, torch.bfloat16):
        raise TypeError("mwer_loss: %s input is not supported: call .float() on it" % input.dtype)
    if input.dtype not in (torch.float32, torch.float64):
        raise TypeError("mwer_loss: input must be float32 or float64, not %s" % input.dtype)
    if input.dim() != 3:
        raise ValueError("mwer_loss: input must be [T, N, C], got %d dimensions" % input.dim())
    if reduction not in _REDUCTIONS:
        raise ValueError("mwer_loss: %r is not a reduction (none, mean, sum)" % (reduction,))
    T, N, C = input.shape
    if C < 1:
        raise ValueError("mwer_loss: empty alphabet")
    if not 0 <= int(blank) < C:
        raise ValueError("mwer_loss: blank %d outside [0, %d)" % (blank, C))
    scale = float(scale)
    if not np.isfinite(scale) or scale < 0:
        raise ValueError("mwer_loss: scale must be finite and >= 0, got %r" % scale)
    if not isinstance(hyps, torch.Tensor):
        raise TypeError("mwer_loss: hyps must be a tensor")
    if hyps.is_floating_point() or hyps.is_complex() or hyps.dtype == torch.bool:
        raise TypeError("mwer_loss: hyps must hold integers, not %s" % hyps.dtype)
    if hyps.dim() != 3 or hyps.shape[0] != N:
        raise ValueError("mwer_loss: hyps must be [N, K, S] with N = %d, got %s" % (N, tuple(hyps.shape)))
    K, S = int(hyps.shape[1]), int(hyps.shape[2])
    if not 1 <= K <= MWER_MAX_K:
        raise ValueError("mwer_loss: K = %d hypotheses outside 1..%d" % (K, MWER_MAX_K))
    if T * N * K > 2 ** 31 - 1:
        raise ValueError("mwer_loss: T * N * K = %d rows do not fit the kernels' int32 row index" % (T * N * K))
    T_n = _host_lengths(input_lengths, N, "input_lengths")
    if T_n.size and (T_n.min() < 1 or T_n.max() > T):
        raise ValueError("mwer_loss: input_lengths must lie in [1, %d]" % T)
    if hyp_counts is None:
        K_n = np.full(N, K, dtype=np.int64)
    else:
        K_n = _host_lengths(hyp_counts, N, "hyp_counts")
        if K_n.size and (K_n.min() < 0 or K_n.max() > K):
            raise ValueError("mwer_loss: hyp_counts must lie in [0, %d]" % K)
    U = _host_matrix(hyp_lengths, (N, K), "hyp_lengths", True)
    W = _host_matrix(errors, (N, K), "errors", False)
    tg = hyps.detach().cpu().numpy()
    read = (np.arange(K)[None, :] < K_n[:, None]) & np.isfinite(W) & (T_n >= 2)[:, None]
    if read.any() and (U[read].min() < 0 or U[read].max() > S):
        raise ValueError("mwer_loss: hyp_lengths must lie in [0, %d]" % S)
    full = read & (U >= 1)
    labels = tg[full[:, :, None] & (np.arange(S)[None, None, :] < U[:, :, None])]       # in (n, k, position) order
    if labels.size and (labels.min() < 0 or labels.max() >= C):
        raise ValueError("mwer_loss: a hypothesis label lies outside [0, %d)" % C)
    if labels.size and (labels == int(blank)).any():
        raise ValueError("mwer_loss: a hypothesis holds the blank (%d)" % blank)
    return (T_n.astype(np.int32), K_n.astype(np.int32), W, full, read & (U == 0),
            np.ascontiguousarray(labels, dtype=np.int32), np.where(full, U, 0).astype(np.int32))


def _mwer_reduce(losses, reduction):
    if reduction == "none":
        return losses
    return losses.sum() if reduction == "sum" else losses.mean()


def _mwer_cfg(x, K, mode, scale, subtract_mean):
    T, N, C = x.shape
    st, sn, sc = x.stride()
    return _sctc.MwerConfig(T, N, K, C, _sctc.F64 if x.dtype == torch.float64 else _sctc.F32, mode, st, sn, sc,
                            float(scale), int(bool(subtract_mean)))


class _MwerLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, host, blank, scale, reduction, subtract_mean, logits):
        T_n, K_n, W, full, empty, labels, U = host
        T, N, C = input.shape
        K = full.shape[1]
        dev = input.device
        L = _sctc.lib()
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = _sctc.current_stream_ptr()
            T_dev = torch.from_numpy(T_n).to(dev)
            K_dev = torch.from_numpy(K_n).to(dev)
            W_dev = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
            mode = _sctc.TNC_LOGITS if logits else _sctc.TNC_LOG_PROBS
            cfg = _mwer_cfg(input, K, mode, scale, subtract_mean)
            # the two K-fold buffers: frame t of hypothesis k of utterance n is row (t * N + n) * K + k
            probs = torch.empty((T * N * K, C), dtype=input.dtype, device=dev)
            grad = torch.empty_like(probs)
            cost = torch.full((N * K,), float("inf"), **f64)        # the pairs no CTC call is made for: not real
            skip = torch.ones(N * K, **i32)
            _sctc.check(L.sctc_ctc_mwer_probs(ctypes.byref(cfg), input.data_ptr(), T_dev.data_ptr(), K_dev.data_ptr(),
                                              probs.data_ptr(), stream), "ctc_mwer_probs")
            pairs = np.flatnonzero(full.reshape(-1))
            if pairs.size:
                rowbase = torch.arange(T, dtype=torch.int32, device=dev) * (N * K)
                whole = pairs.size == N * K
                cost_b = cost if whole else torch.empty(pairs.size, **f64)
                skip_b = skip if whole else torch.empty(pairs.size, **i32)
                T_b = np.ascontiguousarray(np.repeat(T_n, K)[pairs])
                U_b = np.ascontiguousarray(U.reshape(-1)[pairs])
                f_off = np.ascontiguousarray(pairs, dtype=np.int64)
                l_off = np.zeros(pairs.size, dtype=np.int64)
                l_off[1:] = np.cumsum(U_b, dtype=np.int64)[:-1]
                bt = _sctc.CtcBatch(int(pairs.size), C, blank, cfg.dtype, C, _sctc.i32(T_b), _sctc.i32(U_b),
                                    _sctc.i64(f_off), _sctc.i32(labels), _sctc.i64(l_off),
                                    ctypes.c_void_p(rowbase.data_ptr()))
                nbytes = L.sctc_ctc_workspace_bytes(ctypes.byref(bt))
                if nbytes == 0:
                    _sctc.check(-1, "mwer_loss")
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _sctc.check(L.sctc_ctc_loss_batch(ctypes.byref(bt), probs.data_ptr(), grad.data_ptr(), cost_b.data_ptr(),
                                                  skip_b.data_ptr(), ws.data_ptr(), nbytes, stream), "mwer_loss")
                if not whole:
                    at = torch.from_numpy(f_off).to(dev)
                    cost[at] = cost_b
                    skip[at] = skip_b
                del ws
            blanks = np.flatnonzero(empty.reshape(-1))
            if blanks.size:
                # an all-blank hypothesis is a legitimate n-best entry: the buffer as a [T, N * K, C] batch of the
                # empty-target kernel
                tnc = _sctc.TncConfig(T, N * K, C, cfg.dtype, mode, blank, 0, 0, 0)
                T_rep = T_dev.repeat_interleave(K)
                idx = torch.from_numpy(np.ascontiguousarray(blanks, dtype=np.int32)).to(dev)
                _sctc.check(L.sctc_ctc_tnc_empty(ctypes.byref(tnc), probs.data_ptr(), T_rep.data_ptr(), idx.data_ptr(),
                                                 None, int(blanks.size), grad.data_ptr(), cost.data_ptr(),
                                                 skip.data_ptr(), stream), "ctc_tnc_empty")
            loss = torch.empty(N, **f64)
            coef = torch.empty(N * K, **f64)
            post = torch.empty(N * K, **f64)
            expected = torch.empty(N, **f64)
            real = torch.empty(N * K, **i32)
            inactive = torch.empty(N, **i32)
            _sctc.check(L.sctc_ctc_mwer_coef(ctypes.byref(cfg), cost.data_ptr(), skip.data_ptr(), W_dev.data_ptr(),
                                             T_dev.data_ptr(), K_dev.data_ptr(), loss.data_ptr(), coef.data_ptr(),
                                             post.data_ptr(), expected.data_ptr(), real.data_ptr(), inactive.data_ptr(),
                                             stream), "ctc_mwer_coef")
            if ctx.needs_input_grad[0]:
                G = torch.empty((T * N, C), dtype=input.dtype, device=dev)
                _sctc.check(L.sctc_ctc_mwer_combine(ctypes.byref(cfg), probs.data_ptr(), grad.data_ptr(), coef.data_ptr(),
                                                    real.data_ptr(), T_dev.data_ptr(), inactive.data_ptr(), G.data_ptr(),
                                                    stream), "ctc_mwer_combine")
                ctx.save_for_backward(G, T_dev, inactive)
                ctx.meta = (tuple(input.shape), input.dtype, blank, reduction)
            del probs, grad         # the two K-fold buffers end here; backward needs the one [T * N][C] tensor
            is_real = real.reshape(N, K) != 0
            loglik = torch.where(is_real, -cost.reshape(N, K), torch.full((), float("-inf"), **f64))
            out = _mwer_reduce(loss.to(input.dtype), reduction)
            stats = (loglik, post.reshape(N, K), expected, is_real)
            ctx.mark_non_differentiable(*stats)
            return (out,) + stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, *unused):
        G, T_dev, inactive = ctx.saved_tensors
        shape, dtype, blank, reduction = ctx.meta
        N = shape[1]
        with torch.cuda.device(G.device):
            go = grad_output.to(torch.float64)
            if reduction == "none":
                scale = go.reshape(N)
            else:
                scale = (go.reshape(()) / (N if reduction == "mean" else 1)).expand(N)
            scale = scale.contiguous()
            out = torch.empty(shape, dtype=dtype, device=G.device)
            cfg = _cfg(out, _sctc.TNC_LOG_PROBS, blank)
            zero = torch.zeros(N, dtype=torch.float64, device=G.device)
            _sctc.check(_sctc.lib().sctc_ctc_tnc_grad(ctypes.byref(cfg), G.data_ptr(), T_dev.data_ptr(), zero.data_ptr(),
                                                      inactive.data_ptr(), scale.data_ptr(), out.data_ptr(),
                                                      _sctc.current_stream_ptr()), "ctc_tnc_grad")
        return out, None, None, None, None, None, None


def mwer_loss(input, hyps, hyp_lengths, errors, input_lengths, hyp_counts=None, blank=0, scale=1.0, reduction="mean",
              subtract_mean=True, logits=False, return_stats=False):
    host = _mwer_check_args(input, hyps, hyp_lengths, errors, input_lengths, hyp_counts, blank, scale, reduction)
    if not input.is_cuda:
        _sctc.require_gpu()
        raise _sctc.SctcError("mwer_loss: input lives on %s: the CTC kernels have no CPU fallback" % input.device)
    out = _MwerLoss.apply(input, host, int(blank), float(scale), reduction, bool(subtract_mean), bool(logits))
    if not return_stats:
        return out[0]
    return out[0], dict(loglik=out[1].detach(), posterior=out[2].detach(), expected=out[3].detach(), real=out[4].detach())


mwer_loss.__doc__ = _MWER_DOC + """
``input``: a CUDA tensor ``[T, N, C]``, float32 or float64, any strides, as for :func:`ctc_loss`.  ``hyps``: an integer
tensor ``[N, K, S]``, padded, on the CPU or the device; it goes to the host like ``targets`` does.  ``hyp_lengths``:
``[N, K]``.  ``errors``: ``[N, K]``, any real dtype.  ``hyp_counts``: ``[N]``, or None for K everywhere.  Limits:
``1 <= K <= 256``; ``T * N * K <= INT32_MAX``; ``scale`` finite and ``>= 0``.  Every argument error is raised on the host
before the GPU is touched.

``reduction`` "none" gives ``[N]``, "sum" the sum, "mean" the mean over all N; inactive utterances count as 0.  The dtype
is the input's.  ``return_stats=True`` adds a dict of detached device tensors: ``loglik [N, K]`` (-inf where not real),
``posterior [N, K]``, ``expected [N]`` and ``real [N, K]`` (bool).

Backward is once-differentiable and keeps one ``[T * N][C]`` tensor, nothing K-fold; the cost of the call is K-fold
traffic for the probabilities and the gradient rows (DESIGN.md §4.16).
"""


class MWERLoss(torch.nn.Module):
    """:func:`mwer_loss` as a module; ``forward(input, hyps, hyp_lengths, errors, input_lengths, hyp_counts=None)``."""

    def __init__(self, blank=0, scale=1.0, reduction="mean", subtract_mean=True, logits=False):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError("MWERLoss: %r is not a reduction (none, mean, sum)" % (reduction,))
        if not np.isfinite(float(scale)) or float(scale) < 0:
            raise ValueError("MWERLoss: scale must be finite and >= 0, got %r" % (scale,))
        self.blank = blank
        self.scale = scale
        self.reduction = reduction
        self.subtract_mean = subtract_mean
        self.logits = logits

    def forward(self, input, hyps, hyp_lengths, errors, input_lengths, hyp_counts=None):
        return mwer_loss(input, hyps, hyp_lengths, errors, input_lengths, hyp_counts, self.blank, self.scale,
                         self.reduction, self.subtract_mean, self.logits)


def mwer_nbest(input, input_lengths, references, reference_lengths, nbest, beam=40, unit="word", space=None, lm=None,
               alpha=1.0, beta=0.0, logits=False, blank=0):
    """The n-best lists and their errors that :func:`mwer_loss` takes, from the prefix beam search on ``input`` itself:
    a convenience that runs under ``no_grad`` through existing calls only.  Packed log-probabilities ``[sum T][C]`` are
    formed with torch ops (``log_softmax`` first when ``logits``), ``ctc_fast.decode_beam_batch(..., nbest=nbest)``
    searches them, the ranks whose score is ``-inf`` are dropped (``hyp_counts``), and the errors against ``references``
    (``[N, S]`` padded, with ``reference_lengths``) come from ``ctc_fast.edit_distance_batch`` (``unit="char"``) or
    ``ctc_fast.word_errors_batch`` (``unit="word"``, ``space`` required).  Returns ``(hyps [N, K, S] int64, hyp_lengths
    [N, K], hyp_counts [N], errors float64 [N, K])`` on the CPU, K = nbest.  The search's blank is symbol 0: any other
    ``blank`` is a ValueError."""
    import ctc_fast
    if int(blank) != 0:
        raise ValueError("mwer_nbest: the beam search's blank is symbol 0, not %d" % blank)
    if unit not in ("char", "word"):
        raise ValueError("mwer_nbest: unit must be 'char' or 'word', not %r" % (unit,))
    if not isinstance(input, torch.Tensor) or input.dim() != 3:
        raise ValueError("mwer_nbest: input must be a [T, N, C] tensor")
    T, N, C = input.shape
    K = int(nbest)
    if not 1 <= K <= MWER_MAX_K:
        raise ValueError("mwer_nbest: nbest = %d outside 1..%d" % (K, MWER_MAX_K))
    if unit == "word" and (space is None or not 1 <= int(space) < C):
        raise ValueError("mwer_nbest: the word unit needs the space symbol, in [1, %d)" % C)
    T_n = _host_lengths(input_lengths, N, "input_lengths")
    if T_n.size and (T_n.min() < 1 or T_n.max() > T):
        raise ValueError("mwer_nbest: input_lengths must lie in [1, %d]" % T)
    if not isinstance(references, torch.Tensor) or references.dim() != 2 or references.shape[0] != N:
        raise ValueError("mwer_nbest: references must be an [N, S] tensor")
    R_n = _host_lengths(reference_lengths, N, "reference_lengths")
    if R_n.size and (R_n.min() < 0 or R_n.max() > references.shape[1]):
        raise ValueError("mwer_nbest: reference_lengths must lie in [0, %d]" % references.shape[1])
    ref = references.detach().cpu().numpy()
    refs = [np.ascontiguousarray(ref[n, :R_n[n]], dtype=np.int32) for n in range(N)]
    if not input.is_cuda:
        _sctc.require_gpu()
        raise _sctc.SctcError("mwer_nbest: input lives on %s: the beam search has no CPU fallback" % input.device)
    with torch.no_grad():
        lp = input.detach().log_softmax(2) if logits else input.detach()
        packed = torch.cat([lp[:int(T_n[n]), n] for n in range(N)], dim=0).contiguous()
        rows, scores = ctc_fast.decode_beam_batch(packed, [int(t) for t in T_n], beam=beam, alpha=alpha, beta=beta, lm=lm,
                                                  nbest=K)
    if K == 1:
        rows, scores = [[r] for r in rows], np.asarray(scores).reshape(N, 1)
    kept = [[np.asarray(rows[n][k], dtype=np.int64) for k in range(K) if scores[n, k] != float("-inf")] for n in range(N)]
    S = max([1] + [len(h) for row in kept for h in row])
    hyps = np.zeros((N, K, S), dtype=np.int64)
    lengths = np.zeros((N, K), dtype=np.int64)
    counts = np.array([len(row) for row in kept], dtype=np.int64)
    errors = np.zeros((N, K), dtype=np.float64)
    flat, owner = [], []
    for n, row in enumerate(kept):
        for k, h in enumerate(row):
            hyps[n, k, :len(h)] = h
            lengths[n, k] = len(h)
            flat.append(h.astype(np.int32))
            owner.append(n)
    if flat:
        if unit == "char":
            dist = ctc_fast.edit_distance_batch(refs, flat, a_index=owner)[:, 0]
        else:
            dist = ctc_fast.word_errors_batch([refs[n] for n in owner], flat, int(space), A=C)[:, 0]
        at = 0
        for n, row in enumerate(kept):
            errors[n, :len(row)] = dist[at:at + len(row)]
            at += len(row)
    return torch.from_numpy(hyps), torch.from_numpy(lengths), torch.from_numpy(counts), torch.from_numpy(errors)
