"""Delay-penalized RNN-T loss (Kang et al., "Delay-penalized transducer for low-latency streaming ASR", 2022; k2's
`delay_penalty` with rnnt_type="regular") and the expected frame at which each label is emitted, over libwarprnnt_delay.so
(include/rnnt_delay.h).

The lattice is `rnnt_loss`'s; the label edge of row (t, u) carries the bias delay_penalty * ((T_b - 1) / 2 - t), so paths
that emit early weigh more and the gradient pulls the emissions forward.  The returned cost includes the penalty term, as
k2's does; delay_penalty = 0 is the plain loss.  The recipe:

    loss = DelayPenalizedRNNTLoss(blank=0, delay_penalty=0.01)(logits, labels, act_lens, label_lens)
    _, frames = expected_emit_frames(logits, labels, act_lens, label_lens)    # (N, U - 1): the posterior mean frame per label
    latency = (frames.sum(1) / label_lens.clamp(min=1)).mean()                # what one monitors while training for latency

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C
import math

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side

__all__ = ["rnnt_loss_delay", "DelayPenalizedRNNTLoss", "expected_emit_frames", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_delay": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_loss_delay": (C.c_int, [_P, C.c_float, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _lib.rnntOptions,
                                          C.c_int]),
    "compute_rnnt_loss_delay_fwd": (C.c_int, [_P, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _lib.rnntOptions,
                                              C.c_int, C.c_int]),
    "compute_rnnt_loss_delay_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_delay.so", "the delay-penalized loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_delay", maxT, maxU, minibatch, dtype_code)


def _certify(logits, labels, act_lens, label_lens, blank, delay_penalty, validate):
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  "the delay-penalized loss runs on the GPU only: logits are on %(device)s")
    U, A = logits.shape[2], logits.shape[3]
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    if not math.isfinite(float(delay_penalty)):
        raise ValueError("delay_penalty must be finite")


class _DelayPenalized(Function):
    """Two-phase (compute_rnnt_loss_delay_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, blank, delay_penalty, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, blank, delay_penalty, validate)
        B, T, U, A = logits.shape
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_rnnt_loss_delay_fwd(logits.data_ptr(), float(delay_penalty), lab_ptr, label_lens.data_ptr(),
                                                     act_lens.data_ptr(), A, B, costs, None, ws,
                                                     _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.blank = int(blank)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, code), reduction, call,
                             "compute_rnnt_loss_delay_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_rnnt_loss_delay_bwd(logits.data_ptr(), grads, scale, A, B, ws,
                                                     _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_rnnt_loss_delay_bwd")
        return grads, None, None, None, None, None, None, None


def rnnt_loss_delay(acts, labels, act_lens, label_lens, blank=0, delay_penalty=0.0, reduction="mean", validate=True):
    """Delay-penalized RNN-T loss of raw logits (N, T, U, A) with one softmax over all A columns, blank in column `blank`
    (any column).  labels (N, U - 1), act_lens, label_lens (N,) int32 on the device of the logits.  delay_penalty: any
    finite number (it crosses the C-ABI as a float); 0 is the plain RNN-T loss, a negative one rewards late emission.  Costs
    float32 (float64 for float64 logits), the penalty term included; reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.
    validate=False skips every check that reads device memory: the call then only enqueues."""
    _side.check_reduction(reduction)
    return _DelayPenalized.apply(acts, labels, act_lens, label_lens, blank, delay_penalty, reduction, validate)


def expected_emit_frames(acts, labels, act_lens, label_lens, blank=0, delay_penalty=0.0, validate=True):
    """(costs (N,), frames (N, U - 1)) of the costs' type: frames[b, u] is the posterior mean, under the loss's (tilted) path
    distribution, of the frame at which label u of sample b is emitted -- nondecreasing in u, inside [0, T_b - 1], exact 0
    behind a sample's labels.  One forward call, outside autograd (nothing is kept for a backward).  As a seed for the
    alignment-restricted loss: alignment_windows(frames.round().int(), left, right) (warprnnt_pytorch.ar)."""
    logits = acts.detach()
    _certify(logits, labels, act_lens, label_lens, blank, delay_penalty, validate)
    B, T, U, A = logits.shape
    code, dev = _DT[logits.dtype], logits.device
    cdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
    with torch.cuda.device(dev):
        costs = torch.empty(B, dtype=cdt, device=dev)
        frames = torch.empty((B, U - 1), dtype=cdt, device=dev)
        ws = torch.empty(workspace_bytes(T, U, B, code), dtype=torch.uint8, device=dev)
        lab_ptr = labels.data_ptr() if labels.numel() else costs.data_ptr()    # maxU == 1: never read
        _lib.check(lib().compute_rnnt_loss_delay_fwd(logits.data_ptr(), float(delay_penalty), lab_ptr, label_lens.data_ptr(),
                                                     act_lens.data_ptr(), A, B, costs.data_ptr(),
                                                     frames.data_ptr() if frames.numel() else None, ws.data_ptr(),
                                                     _side.options(dev, blank, T, U), code, 0),
                   "compute_rnnt_loss_delay_fwd")
        ws.record_stream(torch.cuda.current_stream(dev))
    return costs, frames


class DelayPenalizedRNNTLoss(Module):
    """Module form of `rnnt_loss_delay`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, blank=0, delay_penalty=0.0, reduction="mean"):
        super().__init__()
        _side.check_reduction(reduction)
        if not math.isfinite(float(delay_penalty)):
            raise ValueError("delay_penalty must be finite")
        self.blank, self.delay_penalty, self.reduction = int(blank), float(delay_penalty), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_delay(acts, labels, act_lens, label_lens, self.blank, self.delay_penalty, self.reduction)
