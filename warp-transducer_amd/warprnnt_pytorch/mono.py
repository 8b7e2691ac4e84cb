"""Monotonic (one label per frame) transducer loss (Tripathi et al., "Monotonic RNN-T", ASRU 2019; k2's
rnnt_type="modified") over libwarprnnt_mono.so (include/rnnt_mono.h).

A label edge consumes a frame as a blank edge does, (t, u) -> (t + 1, u + 1): every alignment emits at most one label per
frame, which is what a streaming decoder with that limit sees.  The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A) raw logits, one softmax over all A columns
    loss = MonotonicRNNTLoss(blank=0)(logits, labels, act_lens, label_lens)

A sample needs T_b >= L_b frames; with fewer it has no alignment.

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side

__all__ = ["rnnt_loss_mono", "MonotonicRNNTLoss", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_mono": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_loss_mono": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int]),
    "compute_rnnt_loss_mono_fwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int, C.c_int]),
    "compute_rnnt_loss_mono_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_mono.so", "the monotonic loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_mono", maxT, maxU, minibatch, dtype_code)


def check_paths(act_lens, label_lens):
    """Every sample has an alignment: T_b >= L_b (one frame per label at least).  Reads the lengths back."""
    short = torch.nonzero(act_lens < label_lens).flatten().tolist()
    if short:
        b = short[0]
        raise ValueError("sample %d has %d frames for %d labels: the monotonic loss emits at most one label per frame"
                         % (b, int(act_lens[b]), int(label_lens[b])))


def _certify(logits, labels, act_lens, label_lens, blank, validate):
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  "the monotonic loss runs on the GPU only: logits are on %(device)s")
    U, A = logits.shape[2], logits.shape[3]
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    if validate:
        check_paths(act_lens, label_lens)


class _Monotonic(Function):
    """Two-phase (compute_rnnt_loss_mono_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, blank, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, blank, validate)
        B, T, U, A = logits.shape
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_rnnt_loss_mono_fwd(logits.data_ptr(), lab_ptr, label_lens.data_ptr(), act_lens.data_ptr(), A,
                                                    B, costs, ws, _side.options(logits.device, blank, T, U), code,
                                                    prepare_backward)
        ctx.blank = int(blank)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, code), reduction, call,
                             "compute_rnnt_loss_mono_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_rnnt_loss_mono_bwd(logits.data_ptr(), grads, scale, A, B, ws,
                                                    _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_rnnt_loss_mono_bwd")
        return grads, None, None, None, None, None, None


def rnnt_loss_mono(acts, labels, act_lens, label_lens, blank=0, reduction="mean", validate=True):
    """Monotonic transducer loss of raw logits (N, T, U, A) with one softmax over all A columns, blank in column `blank`
    (any column).  labels (N, U - 1), act_lens, label_lens (N,) int32 on the device of the logits.  Costs float32 (float64
    for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.  validate=True reads the lengths back and raises
    ValueError for a sample with fewer frames than labels (it has no alignment); validate=False skips every check that
    reads device memory: the call then only enqueues, and such a sample costs +inf."""
    _side.check_reduction(reduction)
    return _Monotonic.apply(acts, labels, act_lens, label_lens, blank, reduction, validate)


class MonotonicRNNTLoss(Module):
    """Module form of `rnnt_loss_mono`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        _side.check_reduction(reduction)
        self.blank, self.reduction = int(blank), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_mono(acts, labels, act_lens, label_lens, self.blank, self.reduction)
