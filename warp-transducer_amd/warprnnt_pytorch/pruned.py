"""Pruned RNN-T loss (Kuang et al., Interspeech 2022) over libwarprnnt_pruned.so (include/rnnt_pruned.h).

The recipe:

    simple = RNNTLossAdd()(am_proj, lm_proj, labels, act_lens, label_lens)          # trivial additive joiner
    ranges = prune_ranges(am_proj, lm_proj, labels, act_lens, label_lens, S)        # (N, T) int32, no gradient
    am_p, lm_p = prune_inputs(am, lm, ranges, S)                                     # (N, T, S, D) each
    logits = joiner(am_p, lm_p)                                                      # (N, T, S, A): the real joiner, S states only
    loss = RNNTLossPruned()(logits, labels, act_lens, label_lens, ranges)

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

__all__ = ["rnnt_loss_pruned", "RNNTLossPruned", "prune_ranges", "prune_inputs", "library_path"]

_DT = {torch.float32: _lib.DT_F32, torch.float64: _lib.DT_F64, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}
_P = C.c_void_p
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
_handle = None


def library_path():
    """Next to libwarprnnt.so: WARP_RNNT_PATH (a directory, or the main library's file), the installed package, the source tree."""
    return os.path.join(os.path.dirname(_lib.library_path()), "libwarprnnt_pruned.so")


def lib():
    global _handle
    if _handle is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError("libwarprnnt_pruned.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                              "There is no fallback for the pruned loss." % path)
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
        _lib.check(lib().get_workspace_size_pruned(int(maxT), int(maxU), int(minibatch), int(dtype_code), C.byref(c)),
                   "get_workspace_size_pruned")
        n = _WS[key] = c.value
    return n


def _options(dev, blank, T, U):
    return _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream,
                            blank_label=int(blank), maxT=int(T), maxU=int(U), batch_first=True)


def _certify(logits, labels, act_lens, label_lens, ranges, validate):
    check_type(labels, torch.int32, "labels")
    check_type(label_lens, torch.int32, "label_lengths")
    check_type(act_lens, torch.int32, "lengths")
    check_type(ranges, torch.int32, "ranges")
    for var, name in ((logits, "logits"), (labels, "labels"), (act_lens, "lengths"), (label_lens, "label_lengths"),
                      (ranges, "ranges")):
        check_contiguous(var, name)
    check_dim(logits, 4, "logits")
    check_dim(labels, 2, "labels")
    check_dim(act_lens, 1, "lengths")
    check_dim(label_lens, 1, "label_lengths")
    check_dim(ranges, 2, "ranges")
    if not logits.is_cuda:
        raise ValueError("the pruned loss runs on the GPU only")
    if logits.dtype not in _DT:
        raise TypeError("logits must be torch.float32, float64, bfloat16 or float16")
    B, T = logits.shape[0], logits.shape[1]
    if act_lens.shape[0] != B or label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a length per example.")
    if tuple(ranges.shape) != (B, T):
        raise ValueError("ranges must be (N, T) = %s, got %s" % ((B, T), tuple(ranges.shape)))
    check_gpu_arguments(logits, labels, act_lens, label_lens)
    if not ranges.is_cuda or ranges.device != logits.device:
        raise ValueError("ranges must be on the device of the logits")
    S = logits.shape[2]
    if S < 1 or S > labels.shape[1] + 1:
        raise ValueError("the window size S = logits.shape[2] must be in [1, maxU], maxU = labels.shape[1] + 1")
    if validate:
        max_t, max_l = torch.stack((act_lens, label_lens)).amax(1).tolist()
        if T != max_t:
            raise ValueError("Input length mismatch")
        if labels.shape[1] != max_l:
            raise ValueError("Output length mismatch")


class _RNNTPruned(Function):
    """Two-phase (compute_rnnt_loss_pruned_fwd / _bwd): the forward call leaves the workspace, the backward call streams the
    gradient once with grad_output and the 1/N of 'mean' folded into its per-sample scale."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, ranges, blank, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, ranges, validate)
        B, T, S, V = logits.shape
        U = labels.shape[1] + 1
        dev = logits.device
        need_grad = logits.requires_grad
        cdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            costs = torch.empty(B, dtype=cdt, device=dev)
            ws = torch.empty(workspace_bytes(T, U, B, _DT[logits.dtype]), dtype=torch.uint8, device=dev)
            lab_ptr = labels.data_ptr() if labels.numel() else costs.data_ptr()    # maxU == 1: never read
            st = lib().compute_rnnt_loss_pruned_fwd(logits.data_ptr(), ranges.data_ptr(), S, lab_ptr, label_lens.data_ptr(),
                                                    act_lens.data_ptr(), V, B, costs.data_ptr(), ws.data_ptr(),
                                                    _options(dev, blank, T, U), _DT[logits.dtype], 1 if need_grad else 0)
            _lib.check(st, "compute_rnnt_loss_pruned_fwd")
        ctx.save_for_backward(logits)
        ctx.workspace = ws if need_grad else None
        ctx.blank, ctx.U = int(blank), U
        ctx.mean_scale = 1.0 / B if reduction == "mean" else 1.0
        if reduction == "sum":
            return costs.sum(0, keepdim=True)
        if reduction == "mean":
            return costs.mean(0, keepdim=True)
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, S, V = logits.shape
        dev = logits.device
        sdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            scale = (grad_output.reshape(-1).to(device=dev, dtype=sdt).expand(B) * ctx.mean_scale).contiguous()
            grads = torch.empty_like(logits)
            st = lib().compute_rnnt_loss_pruned_bwd(logits.data_ptr(), grads.data_ptr(), scale.data_ptr(), S, V, B,
                                                    ctx.workspace.data_ptr(), _options(dev, ctx.blank, T, ctx.U),
                                                    _DT[logits.dtype])
            _lib.check(st, "compute_rnnt_loss_pruned_bwd")
            ctx.workspace.record_stream(torch.cuda.current_stream(dev))
        return grads, None, None, None, None, None, None, None


def rnnt_loss_pruned(logits, labels, act_lens, label_lens, ranges, blank=0, reduction="mean", validate=True):
    """Pruned RNN-T loss of raw logits (N, T, S, A): row (b, t, k) is the joint output of lattice state ranges[b, t] + k.
    labels (N, maxU - 1), act_lens, label_lens (N,) int32 and ranges (N, T) int32, on the device of the logits.  Costs float32
    (float64 for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.  validate=False skips the checks that
    read the lengths back (T == max(act_lens), labels.shape[1] == max(label_lens)): the call then only enqueues."""
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
                                                 _options(dev, blank, T, U), _RANGES_DT[trans_acts.dtype])
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
