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
