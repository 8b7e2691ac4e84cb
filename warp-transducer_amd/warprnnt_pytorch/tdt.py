"""Token-and-Duration Transducer (TDT) loss (Xu et al., ICML 2023) over libwarprnnt_tdt.so (include/rnnt_tdt.h).

The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A + D): A token logits (blank included), D duration logits
    loss = TDTLoss(durations=[0, 1, 2, 3, 4], blank=A - 1, sigma=0.05)(logits, labels, act_lens, label_lens)

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

__all__ = ["rnnt_loss_tdt", "TDTLoss", "library_path"]

_DT = {torch.float32: _lib.DT_F32, torch.float64: _lib.DT_F64, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}
_P = C.c_void_p
EXPORTS = {
    "get_workspace_size_tdt": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_tdt_loss": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                   _lib.rnntOptions, C.c_int]),
    "compute_tdt_loss_fwd": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions,
                                       C.c_int, C.c_int]),
    "compute_tdt_loss_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_handle = None


def library_path():
    """Next to libwarprnnt.so: WARP_RNNT_PATH (a directory, or the main library's file), the installed package, the source tree."""
    return os.path.join(os.path.dirname(_lib.library_path()), "libwarprnnt_tdt.so")


def lib():
    global _handle
    if _handle is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError("libwarprnnt_tdt.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                              "There is no fallback for the TDT loss." % path)
        h = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        _handle = h
    return _handle


_WS = {}


def workspace_bytes(maxT, maxU, minibatch, num_durations, dtype_code):
    key = (maxT, maxU, minibatch, num_durations, dtype_code)
    n = _WS.get(key)
    if n is None:
        c = C.c_size_t(0)
        _lib.check(lib().get_workspace_size_tdt(int(maxT), int(maxU), int(minibatch), int(num_durations), int(dtype_code),
                                                C.byref(c)), "get_workspace_size_tdt")
        n = _WS[key] = c.value
    return n


def durations_array(durations):
    """The host int array of the C-ABI, checked as include/rnnt_tdt.h asks."""
    d = [int(v) for v in durations]
    if not 1 <= len(d) <= 8:
        raise ValueError("1 to 8 durations, got %d" % len(d))
    if d[0] < 0 or any(b <= a for a, b in zip(d, d[1:])) or not 1 <= d[-1] <= 64:
        raise ValueError("durations must be strictly increasing, non-negative, the largest in [1, 64]: %s" % (d,))
    return (C.c_int * len(d))(*d)


def _options(dev, blank, T, U):
    return _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream,
                            blank_label=int(blank), maxT=int(T), maxU=int(U), batch_first=True)


def _certify(logits, labels, act_lens, label_lens, D, blank, validate):
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
        raise ValueError("the TDT loss runs on the GPU only: logits are on %s" % logits.device)
    if logits.dtype not in _DT:
        raise TypeError("logits must be torch.float32, float64, bfloat16 or float16")
    B, T, U = logits.shape[0], logits.shape[1], logits.shape[2]
    if act_lens.shape[0] != B or label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a length per example.")
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    A = logits.shape[3] - D
    if A < 1:
        raise ValueError("logits.shape[3] = %d leaves no token column next to %d durations" % (logits.shape[3], D))
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a token column (A = %d)" % (int(blank), A))
    check_gpu_arguments(logits, labels, act_lens, label_lens)
    if validate:
        max_t, max_l = torch.stack((act_lens, label_lens)).amax(1).tolist()
        if T != max_t:
            raise ValueError("Input length mismatch")
        if labels.shape[1] != max_l:
            raise ValueError("Output length mismatch")
    return A


class _TDT(Function):
    """Two-phase (compute_tdt_loss_fwd / _bwd): the forward call leaves the workspace, the backward call streams the gradient
    once with grad_output and the 1/N of 'mean' folded into its per-sample scale."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, durations, blank, sigma, reduction, validate):
        dur = durations_array(durations)
        D = len(dur)
        A = _certify(logits, labels, act_lens, label_lens, D, blank, validate)
        B, T, U, _ = logits.shape
        dev = logits.device
        need_grad = logits.requires_grad
        cdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            costs = torch.empty(B, dtype=cdt, device=dev)
            ws = torch.empty(workspace_bytes(T, U, B, D, _DT[logits.dtype]), dtype=torch.uint8, device=dev)
            lab_ptr = labels.data_ptr() if labels.numel() else costs.data_ptr()    # maxU == 1: never read
            st = lib().compute_tdt_loss_fwd(logits.data_ptr(), dur, D, float(sigma), lab_ptr, label_lens.data_ptr(),
                                            act_lens.data_ptr(), A, B, costs.data_ptr(), ws.data_ptr(),
                                            _options(dev, blank, T, U), _DT[logits.dtype], 1 if need_grad else 0)
            _lib.check(st, "compute_tdt_loss_fwd")
        ctx.save_for_backward(logits)
        ctx.workspace = ws if need_grad else None
        ctx.dur, ctx.A, ctx.blank = dur, A, int(blank)
        ctx.mean_scale = 1.0 / B if reduction == "mean" else 1.0
        if reduction == "sum":
            return costs.sum(0, keepdim=True)
        if reduction == "mean":
            return costs.mean(0, keepdim=True)
        return costs

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, _ = logits.shape
        dev = logits.device
        sdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            scale = (grad_output.reshape(-1).to(device=dev, dtype=sdt).expand(B) * ctx.mean_scale).contiguous()
            grads = torch.empty_like(logits)
            st = lib().compute_tdt_loss_bwd(logits.data_ptr(), grads.data_ptr(), scale.data_ptr(), ctx.dur, len(ctx.dur),
                                            ctx.A, B, ctx.workspace.data_ptr(), _options(dev, ctx.blank, T, U),
                                            _DT[logits.dtype])
            _lib.check(st, "compute_tdt_loss_bwd")
            ctx.workspace.record_stream(torch.cuda.current_stream(dev))
        return grads, None, None, None, None, None, None, None, None


def rnnt_loss_tdt(acts, labels, act_lens, label_lens, durations, blank=0, sigma=0.0, reduction="mean", validate=True):
    """TDT loss of raw logits (N, T, U, A + D): the first A columns are tokens (blank = `blank`), the last D the logits of
    `durations` (1 to 8 ints, strictly increasing, non-negative, the largest in [1, 64]).  sigma: the logit
    under-normalisation of the token log-probs (natural log).  labels (N, U - 1), act_lens, label_lens (N,) int32 on the
    device of the logits.  Costs float32 (float64 for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.
    validate=False skips the checks that read the lengths back: the call then only enqueues."""
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("reduction must be 'none', 'sum' or 'mean'")
    return _TDT.apply(acts, labels, act_lens, label_lens, tuple(int(d) for d in durations), blank, float(sigma), reduction,
                      validate)


class TDTLoss(Module):
    """Module form of `rnnt_loss_tdt`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, durations, blank=0, sigma=0.0, reduction="mean"):
        super().__init__()
        durations_array(durations)
        self.durations = tuple(int(d) for d in durations)
        self.blank, self.sigma, self.reduction = blank, float(sigma), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_tdt(acts, labels, act_lens, label_lens, self.durations, self.blank, self.sigma, self.reduction)
