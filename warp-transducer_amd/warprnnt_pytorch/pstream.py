"""Pruned RNN-T loss with k2's `rnnt_type` ("regular" | "modified") and `delay_penalty`, over libwarprnnt_pstream.so
(include/rnnt_pstream.h): what a streaming recipe passes to k2's `rnnt_loss_pruned`, on the pruned (N, T, S, A) logits.

The windows, the labels and the lengths are those of `warprnnt_pytorch.pruned`; the lattice type and the bias of the label
edges are those of `warprnnt_pytorch.mono` and `warprnnt_pytorch.delay`.  The recipe:

    ranges = prune_ranges(am_proj, lm_proj, labels, act_lens, label_lens, S)        # warprnnt_pytorch.pruned
    am_p, lm_p = prune_inputs(am, lm, ranges, S)
    logits = joiner(am_p, lm_p)                                                      # (N, T, S, A)
    loss = PrunedStreamingRNNTLoss(rnnt_type="modified", delay_penalty=0.01)(logits, labels, act_lens, label_lens, ranges)

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C
import math

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side
from .pruned import _certify as _certify_pruned

__all__ = ["rnnt_loss_pruned_stream", "PrunedStreamingRNNTLoss", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_pstream": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_loss_pstream": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                            _lib.rnntOptions, C.c_int]),
    "compute_rnnt_loss_pstream_fwd": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                                _lib.rnntOptions, C.c_int, C.c_int]),
    "compute_rnnt_loss_pstream_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_pstream.so", "the pruned streaming loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load

RNNT_TYPES = {"regular": 0, "modified": 1}


def workspace_bytes(maxT, maxU, S, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_pstream", maxT, maxU, S, minibatch, dtype_code)


def type_code(rnnt_type):
    """0 / 1 of include/rnnt_pstream.h for "regular" / "modified"; anything else (k2's "constrained" too) is refused."""
    if not isinstance(rnnt_type, str) or rnnt_type not in RNNT_TYPES:
        raise ValueError("rnnt_type must be 'regular' or 'modified', got %r" % (rnnt_type,))
    return RNNT_TYPES[rnnt_type]


def check_penalty(delay_penalty):
    if not math.isfinite(float(delay_penalty)):
        raise ValueError("delay_penalty must be finite")
    return float(delay_penalty)


def _certify(logits, labels, act_lens, label_lens, ranges, blank, rnnt_type, delay_penalty, validate):
    code = type_code(rnnt_type)
    check_penalty(delay_penalty)
    if isinstance(logits, torch.Tensor) and not logits.is_cuda:
        raise ValueError("the pruned streaming loss runs on the GPU only: logits are on %s" % logits.device)
    _certify_pruned(logits, labels, act_lens, label_lens, ranges, validate)
    if not 0 <= int(blank) < logits.shape[3]:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), logits.shape[3]))
    if validate and code == 1:
        short = torch.nonzero(act_lens < label_lens).flatten().tolist()
        if short:
            b = short[0]
            raise ValueError("rnnt_type='modified' emits at most one label per frame: sample %d has T_b = %d < L_b = %d"
                             % (b, int(act_lens[b]), int(label_lens[b])))
    return code


class _PrunedStream(Function):
    """Two-phase (compute_rnnt_loss_pstream_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, ranges, blank, rnnt_type, delay_penalty, reduction, validate):
        tcode = _certify(logits, labels, act_lens, label_lens, ranges, blank, rnnt_type, delay_penalty, validate)
        B, T, S, A = logits.shape
        U = labels.shape[1] + 1
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_rnnt_loss_pstream_fwd(logits.data_ptr(), ranges.data_ptr(), S, tcode, float(delay_penalty),
                                                       lab_ptr, label_lens.data_ptr(), act_lens.data_ptr(), A, B, costs, ws,
                                                       _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.blank, ctx.U = int(blank), U
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, S, B, code), reduction, call,
                             "compute_rnnt_loss_pstream_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, S, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_rnnt_loss_pstream_bwd(logits.data_ptr(), grads, scale, S, A, B, ws,
                                                       _side.options(logits.device, ctx.blank, T, ctx.U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_rnnt_loss_pstream_bwd")
        return grads, None, None, None, None, None, None, None, None, None


def rnnt_loss_pruned_stream(logits, labels, act_lens, label_lens, ranges, blank=0, rnnt_type="regular", delay_penalty=0.0,
                            reduction="mean", validate=True):
    """Pruned RNN-T loss of raw logits (N, T, S, A): row (b, t, k) is the joint output of lattice state ranges[b, t] + k;
    one softmax over all A columns, blank in column `blank`.  labels (N, maxU - 1), act_lens, label_lens (N,) int32 and
    ranges (N, T) int32, on the device of the logits.  rnnt_type "regular" (a label edge stays in its frame) or "modified"
    (it consumes a frame: at most one label per frame, T_b >= L_b).  delay_penalty: any finite number (it crosses the C-ABI
    as a float); the label edge of frame t carries delay_penalty * ((T_b - 1) / 2 - t), and the cost includes that term, as
    k2's does.  Costs float32 (float64 for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.
    validate=False skips every check that reads device memory: the call then only enqueues."""
    _side.check_reduction(reduction)
    return _PrunedStream.apply(logits, labels, act_lens, label_lens, ranges, blank, rnnt_type, delay_penalty, reduction,
                               validate)


class PrunedStreamingRNNTLoss(Module):
    """Module form of `rnnt_loss_pruned_stream`: forward(logits, labels, act_lens, label_lens, ranges)."""

    def __init__(self, blank=0, rnnt_type="regular", delay_penalty=0.0, reduction="mean", validate=True):
        super().__init__()
        _side.check_reduction(reduction)
        type_code(rnnt_type)
        self.blank, self.rnnt_type, self.delay_penalty = int(blank), rnnt_type, check_penalty(delay_penalty)
        self.reduction, self.validate = reduction, validate

    def forward(self, logits, labels, act_lens, label_lens, ranges):
        return rnnt_loss_pruned_stream(logits, labels, act_lens, label_lens, ranges, self.blank, self.rnnt_type,
                                       self.delay_penalty, self.reduction, self.validate)
