"""Hybrid Autoregressive Transducer (HAT) loss (Variani et al., ICASSP 2020) over libwarprnnt_hat.so (include/rnnt_hat.h).

HAT models blank with a Bernoulli, b = sigmoid(z_blank), and the labels with a softmax over the non-blank columns scaled by
1 - b.  The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A) raw logits, blank in column `blank`
    loss = HATLoss(blank=0)(logits, labels, act_lens, label_lens)

`hat_log_probs(logits, blank)` is the same transform in plain torch, for callers who need the (N, T, U, A) log-probabilities
themselves (internal language model estimation).

The library is a separate shared object, loaded on the first call (`import warprnnt_pytorch` does not need it); a missing
library is an error, there is no fallback.
"""
import ctypes as C
import os

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib
from ._checks import check_contiguous, check_dim, check_type, check_gpu_arguments

__all__ = ["rnnt_loss_hat", "HATLoss", "hat_log_probs", "library_path"]

_DT = {torch.float32: _lib.DT_F32, torch.float64: _lib.DT_F64, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}
_P = C.c_void_p
EXPORTS = {
    "get_workspace_size_hat": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_hat_loss": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int]),
    "compute_hat_loss_fwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int, C.c_int]),
    "compute_hat_loss_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_handle = None


def library_path():
    """Next to libwarprnnt.so: WARP_RNNT_PATH (a directory, or the main library's file), the installed package, the source tree."""
    return os.path.join(os.path.dirname(_lib.library_path()), "libwarprnnt_hat.so")


def lib():
    global _handle
    if _handle is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError("libwarprnnt_hat.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                              "There is no fallback for the HAT loss." % path)
        h = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        _handle = h
    return _handle


_WS = {}


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    key = (maxT, maxU, minibatch, dtype_code)
    n = _WS.get(key)
    if n is None:
        c = C.c_size_t(0)
        _lib.check(lib().get_workspace_size_hat(int(maxT), int(maxU), int(minibatch), int(dtype_code), C.byref(c)),
                   "get_workspace_size_hat")
        n = _WS[key] = c.value
    return n


def hat_log_probs(acts, blank=0):
    """(N, T, U, A) HAT log-probabilities of raw logits, in plain torch (any device, differentiable): column `blank` holds
    log sigmoid(z_blank), column k != blank log(1 - sigmoid(z_blank)) + log_softmax over the non-blank columns.  Every row
    sums to one, so `RNNTLoss` of the result is the HAT loss -- the route this module's kernels replace (it holds a second
    tensor of the logits' size)."""
    A = acts.shape[-1]
    if not 0 <= int(blank) < A or A < 2:
        raise ValueError("blank = %d is not a column of %d >= 2" % (int(blank), A))
    zb = acts[..., blank:blank + 1]
    masked = acts.masked_fill(torch.arange(A, device=acts.device) == int(blank), float("-inf"))
    out = torch.nn.functional.logsigmoid(-zb) + torch.log_softmax(masked, -1)
    return torch.cat((out[..., :blank], torch.nn.functional.logsigmoid(zb), out[..., blank + 1:]), -1)


def _options(dev, blank, T, U):
    return _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream,
                            blank_label=int(blank), maxT=int(T), maxU=int(U), batch_first=True)


def _certify(logits, labels, act_lens, label_lens, blank, validate):
    check_type(labels, torch.int32, "labels")
    check_type(label_lens, torch.int32, "label_lengths")
    check_type(act_lens, torch.int32, "lengths")
    for var, name in ((logits, "logits"), (labels, "labels"), (act_lens, "lengths"), (label_lens, "label_lengths")):
        check_contiguous(var, name)
    check_dim(logits, 4, "logits")
    check_dim(labels, 2, "labels")
    check_dim(act_lens, 1, "lengths")
    check_dim(label_lens, 1, "label_lengths")
    if not logits.is_cuda:
        raise ValueError("the HAT loss runs on the GPU only: logits are on %s" % logits.device)
    if logits.dtype not in _DT:
        raise TypeError("logits must be torch.float32, float64, bfloat16 or float16")
    B, T, U, A = logits.shape
    if act_lens.shape[0] != B or label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a length per example.")
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if A < 2:
        raise ValueError("HAT needs a label column besides the blank: logits.shape[3] = %d" % A)
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    check_gpu_arguments(logits, labels, act_lens, label_lens)
    if validate:
        max_t, max_l = torch.stack((act_lens, label_lens)).amax(1).tolist()
        if T != max_t:
            raise ValueError("Input length mismatch")
        if labels.shape[1] != max_l:
            raise ValueError("Output length mismatch")
        if labels.numel():
            inside = torch.arange(labels.shape[1], device=labels.device) < label_lens.unsqueeze(1)
            if bool(((labels == int(blank)) & inside).any()):
                raise ValueError("a label equals blank = %d: HAT has no label probability for it" % int(blank))


class _HAT(Function):
    """Two-phase (compute_hat_loss_fwd / _bwd): the forward call leaves the workspace, the backward call streams the gradient
    once with grad_output and the 1/N of 'mean' folded into its per-sample scale."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, blank, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, blank, validate)
        B, T, U, A = logits.shape
        dev = logits.device
        need_grad = logits.requires_grad
        cdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            costs = torch.empty(B, dtype=cdt, device=dev)
            ws = torch.empty(workspace_bytes(T, U, B, _DT[logits.dtype]), dtype=torch.uint8, device=dev)
            lab_ptr = labels.data_ptr() if labels.numel() else costs.data_ptr()    # maxU == 1: never read
            st = lib().compute_hat_loss_fwd(logits.data_ptr(), lab_ptr, label_lens.data_ptr(), act_lens.data_ptr(), A, B,
                                            costs.data_ptr(), ws.data_ptr(), _options(dev, blank, T, U),
                                            _DT[logits.dtype], 1 if need_grad else 0)
            _lib.check(st, "compute_hat_loss_fwd")
        ctx.save_for_backward(logits)
        ctx.workspace = ws if need_grad else None
        ctx.blank = int(blank)
        ctx.mean_scale = 1.0 / B if reduction == "mean" else 1.0
        if reduction == "sum":
            return costs.sum(0, keepdim=True)
        if reduction == "mean":
            return costs.mean(0, keepdim=True)
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, A = logits.shape
        dev = logits.device
        sdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            scale = (grad_output.reshape(-1).to(device=dev, dtype=sdt).expand(B) * ctx.mean_scale).contiguous()
            grads = torch.empty_like(logits)
            st = lib().compute_hat_loss_bwd(logits.data_ptr(), grads.data_ptr(), scale.data_ptr(), A, B,
                                            ctx.workspace.data_ptr(), _options(dev, ctx.blank, T, U), _DT[logits.dtype])
            _lib.check(st, "compute_hat_loss_bwd")
            ctx.workspace.record_stream(torch.cuda.current_stream(dev))
        return grads, None, None, None, None, None, None


def rnnt_loss_hat(acts, labels, act_lens, label_lens, blank=0, reduction="mean", validate=True):
    """HAT loss of raw logits (N, T, U, A), blank in column `blank` (any column).  labels (N, U - 1), act_lens, label_lens
    (N,) int32 on the device of the logits; no label may equal `blank`.  Costs float32 (float64 for float64 logits);
    reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.  validate=False skips the checks that read lengths and labels back:
    the call then only enqueues (and a label equal to blank gives its sample a NaN cost instead of a ValueError)."""
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("reduction must be 'none', 'sum' or 'mean'")
    return _HAT.apply(acts, labels, act_lens, label_lens, blank, reduction, validate)


class HATLoss(Module):
    """Module form of `rnnt_loss_hat`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        if reduction not in ("none", "sum", "mean"):
            raise ValueError("reduction must be 'none', 'sum' or 'mean'")
        self.blank, self.reduction = int(blank), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_hat(acts, labels, act_lens, label_lens, self.blank, self.reduction)
