"""Pruned RNN-T loss (Kuang et al., Interspeech 2022) over libwarprnnt_pruned.so (include/rnnt_pruned.h).

The recipe:

    simple = RNNTLossAdd()(am_proj, lm_proj, labels, act_lens, label_lens)          # trivial additive joiner
    ranges = prune_ranges(am_proj, lm_proj, labels, act_lens, label_lens, S)        # (N, T) int32, no gradient
    am_p, lm_p = prune_inputs(am, lm, ranges, S)                                     # (N, T, S, D) each
    logits = joiner(am_p, lm_p)                                                      # (N, T, S, A): the real joiner, S states only
    loss = RNNTLossPruned()(logits, labels, act_lens, label_lens, ranges)

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side
from ._checks import check_contiguous, check_dim, check_type

__all__ = ["rnnt_loss_pruned", "RNNTLossPruned", "prune_ranges", "prune_inputs", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_pruned": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_loss_pruned": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions,
                                           C.c_int]),
    "compute_rnnt_loss_pruned_fwd": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions,
                                               C.c_int, C.c_int]),
    "compute_rnnt_loss_pruned_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
    "compute_rnnt_prune_ranges_add": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _lib.rnntOptions,
                                                C.c_int]),
}
_LIB = _side.Library("libwarprnnt_pruned.so", "the pruned loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_pruned", maxT, maxU, minibatch, dtype_code)


def _certify(logits, labels, act_lens, label_lens, ranges, validate):
    _side.certify(logits, labels, act_lens, label_lens, validate, "the pruned loss runs on the GPU only")
    check_type(ranges, torch.int32, "ranges")
    check_contiguous(ranges, "ranges")
    check_dim(ranges, 2, "ranges")
    B, T, S = logits.shape[0], logits.shape[1], logits.shape[2]
    if tuple(ranges.shape) != (B, T):
        raise ValueError("ranges must be (N, T) = %s, got %s" % ((B, T), tuple(ranges.shape)))
    if not ranges.is_cuda or ranges.device != logits.device:
        raise ValueError("ranges must be on the device of the logits")
    if S < 1 or S > labels.shape[1] + 1:
        raise ValueError("the window size S = logits.shape[2] must be in [1, maxU], maxU = labels.shape[1] + 1")


class _RNNTPruned(Function):
    """Two-phase (compute_rnnt_loss_pruned_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, ranges, blank, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, ranges, validate)
        B, T, S, V = logits.shape
        U = labels.shape[1] + 1
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_rnnt_loss_pruned_fwd(logits.data_ptr(), ranges.data_ptr(), S, lab_ptr, label_lens.data_ptr(),
                                                      act_lens.data_ptr(), V, B, costs, ws,
                                                      _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.blank, ctx.U = int(blank), U
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, code), reduction, call,
                             "compute_rnnt_loss_pruned_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, S, V = logits.shape

        def call(grads, scale, ws):
            return lib().compute_rnnt_loss_pruned_bwd(logits.data_ptr(), grads, scale, S, V, B, ws,
                                                      _side.options(logits.device, ctx.blank, T, ctx.U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_rnnt_loss_pruned_bwd")
        return grads, None, None, None, None, None, None, None


def rnnt_loss_pruned(logits, labels, act_lens, label_lens, ranges, blank=0, reduction="mean", validate=True):
    """Pruned RNN-T loss of raw logits (N, T, S, A): row (b, t, k) is the joint output of lattice state ranges[b, t] + k.
    labels (N, maxU - 1), act_lens, label_lens (N,) int32 and ranges (N, T) int32, on the device of the logits.  Costs float32
    (float64 for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.  validate=False skips the checks that
    read the lengths back (T == max(act_lens), labels.shape[1] == max(label_lens)): the call then only enqueues."""
    # no _side.check_reduction here: an unknown `reduction` has always behaved as 'none'
    return _RNNTPruned.apply(logits, labels, act_lens, label_lens, ranges, blank, reduction, validate)


class RNNTLossPruned(Module):
    def __init__(self, blank=0, reduction="mean", validate=True):
        super().__init__()
        self.blank, self.reduction, self.validate = blank, reduction, validate

    def forward(self, logits, labels, act_lens, label_lens, ranges):
        return rnnt_loss_pruned(logits, labels, act_lens, label_lens, ranges, self.blank, self.reduction, self.validate)


_RANGES_DT = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}


def prune_ranges(trans_acts, pred_acts, labels, act_lens, label_lens, S, blank=0):
    """Window starts (N, T) int32 of S label states per frame from the occupancy of the additive joint
    trans_acts[:, :, None] + pred_acts[:, None] (the lattice of `RNNTLossAdd`; float32, bfloat16 or float16).  The rule is
    include/rnnt_pruned.h's (compute_rnnt_prune_ranges_add).  Enqueued on the current stream; no gradient."""
    from .add_network import _certify as certify_add
    certify_add(trans_acts, pred_acts, labels, act_lens, label_lens)
    if trans_acts.dtype not in _RANGES_DT:
        raise TypeError("trans_acts must be torch.float32, bfloat16 or float16")
    B, T, V = trans_acts.shape
    U = pred_acts.shape[1]
    S = int(S)
    if S < 2 or S > U:
        raise ValueError("S must be in [2, maxU] = [2, %d]" % U)
    dev = trans_acts.device
    with torch.no_grad(), torch.cuda.device(dev):
        ranges = torch.empty((B, T), dtype=torch.int32, device=dev)
        ws = torch.empty(workspace_bytes(T, U, B, _RANGES_DT[trans_acts.dtype]), dtype=torch.uint8, device=dev)
        lab_ptr = labels.data_ptr() if labels.numel() else ranges.data_ptr()
        st = lib().compute_rnnt_prune_ranges_add(trans_acts.data_ptr(), pred_acts.data_ptr(), lab_ptr, label_lens.data_ptr(),
                                                 act_lens.data_ptr(), V, B, S, ranges.data_ptr(), ws.data_ptr(),
                                                 _side.options(dev, blank, T, U), _RANGES_DT[trans_acts.dtype])
        _lib.check(st, "compute_rnnt_prune_ranges_add")
        ws.record_stream(torch.cuda.current_stream(dev))
    return ranges


def prune_inputs(am, lm, ranges, S):
    """The joiner inputs of the pruned positions: am (N, T, D) -> (N, T, S, D) (a broadcast view), lm (N, maxU, D) gathered at
    ranges + arange(S), clamped to maxU - 1 -> (N, T, S, D).  Pure torch; differentiable in am and lm."""
    N, T, D = am.shape
    U = lm.shape[1]
    idx = ranges.long().unsqueeze(-1) + torch.arange(int(S), device=ranges.device)
    idx = idx.clamp_(max=U - 1)                                                   # (N, T, S)
    lm_p = torch.gather(lm.unsqueeze(1).expand(N, T, U, lm.shape[2]), 2,
                        idx.unsqueeze(-1).expand(N, T, int(S), lm.shape[2]))
    return am.unsqueeze(2).expand(N, T, int(S), D), lm_p
