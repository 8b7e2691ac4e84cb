"""Hybrid Autoregressive Transducer (HAT) loss (Variani et al., ICASSP 2020) over libwarprnnt_hat.so (include/rnnt_hat.h).

HAT models blank with a Bernoulli, b = sigmoid(z_blank), and the labels with a softmax over the non-blank columns scaled by
1 - b.  The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A) raw logits, blank in column `blank`
    loss = HATLoss(blank=0)(logits, labels, act_lens, label_lens)

`hat_log_probs(logits, blank)` is the same transform in plain torch, for callers who need the (N, T, U, A) log-probabilities
themselves (internal language model estimation).

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side

__all__ = ["rnnt_loss_hat", "HATLoss", "hat_log_probs", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_hat": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_hat_loss": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int]),
    "compute_hat_loss_fwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int, C.c_int]),
    "compute_hat_loss_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_hat.so", "the HAT loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_hat", maxT, maxU, minibatch, dtype_code)


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


def _certify(logits, labels, act_lens, label_lens, blank, validate):
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  "the HAT loss runs on the GPU only: logits are on %(device)s")
    U, A = logits.shape[2], logits.shape[3]
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if A < 2:
        raise ValueError("HAT needs a label column besides the blank: logits.shape[3] = %d" % A)
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    if validate and labels.numel():
        inside = torch.arange(labels.shape[1], device=labels.device) < label_lens.unsqueeze(1)
        if bool(((labels == int(blank)) & inside).any()):
            raise ValueError("a label equals blank = %d: HAT has no label probability for it" % int(blank))


class _HAT(Function):
    """Two-phase (compute_hat_loss_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, blank, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, blank, validate)
        B, T, U, A = logits.shape
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_hat_loss_fwd(logits.data_ptr(), lab_ptr, label_lens.data_ptr(), act_lens.data_ptr(), A, B,
                                              costs, ws, _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.blank = int(blank)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, code), reduction, call, "compute_hat_loss_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_hat_loss_bwd(logits.data_ptr(), grads, scale, A, B, ws,
                                              _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_hat_loss_bwd")
        return grads, None, None, None, None, None, None


def rnnt_loss_hat(acts, labels, act_lens, label_lens, blank=0, reduction="mean", validate=True):
    """HAT loss of raw logits (N, T, U, A), blank in column `blank` (any column).  labels (N, U - 1), act_lens, label_lens
    (N,) int32 on the device of the logits; no label may equal `blank`.  Costs float32 (float64 for float64 logits);
    reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.  validate=False skips the checks that read lengths and labels back:
    the call then only enqueues (and a label equal to blank gives its sample a NaN cost instead of a ValueError)."""
    _side.check_reduction(reduction)
    return _HAT.apply(acts, labels, act_lens, label_lens, blank, reduction, validate)


class HATLoss(Module):
    """Module form of `rnnt_loss_hat`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        _side.check_reduction(reduction)
        self.blank, self.reduction = int(blank), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_hat(acts, labels, act_lens, label_lens, self.blank, self.reduction)
