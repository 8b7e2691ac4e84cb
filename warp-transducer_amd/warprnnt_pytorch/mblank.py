"""Multi-blank transducer loss (Xu et al., "Multi-blank Transducers for Speech Recognition", ICASSP 2023; NeMo's
MultiblankRNNTLoss) over libwarprnnt_mblank.so (include/rnnt_mblank.h).

Besides the standard blank (one frame) the vocabulary holds K "big blank" columns, each of which consumes a fixed number of
frames.  The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A) raw logits, one softmax over all A columns
    loss = MultiBlankLoss(big_blank_durations=[2, 4, 8], blank=A - 1, sigma=0.05)(logits, labels, act_lens, label_lens)

With `big_blank_columns=None` the columns are NeMo's: big blank i sits in column `blank - 1 - i`.

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

__all__ = ["rnnt_loss_mblank", "MultiBlankLoss", "library_path"]

_DT = {torch.float32: _lib.DT_F32, torch.float64: _lib.DT_F64, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}
_P = C.c_void_p
EXPORTS = {
    "get_workspace_size_mblank": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_mblank_loss": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                      _lib.rnntOptions, C.c_int]),
    "compute_mblank_loss_fwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                          _lib.rnntOptions, C.c_int, C.c_int]),
    "compute_mblank_loss_bwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_handle = None


def library_path():
    """Next to libwarprnnt.so: WARP_RNNT_PATH (a directory, or the main library's file), the installed package, the source tree."""
    return os.path.join(os.path.dirname(_lib.library_path()), "libwarprnnt_mblank.so")


def lib():
    global _handle
    if _handle is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError("libwarprnnt_mblank.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                              "There is no fallback for the multi-blank loss." % path)
        h = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        _handle = h
    return _handle


_WS = {}


def workspace_bytes(maxT, maxU, minibatch, num_big_blanks, dtype_code):
    key = (maxT, maxU, minibatch, num_big_blanks, dtype_code)
    n = _WS.get(key)
    if n is None:
        c = C.c_size_t(0)
        _lib.check(lib().get_workspace_size_mblank(int(maxT), int(maxU), int(minibatch), int(num_big_blanks),
                                                   int(dtype_code), C.byref(c)), "get_workspace_size_mblank")
        n = _WS[key] = c.value
    return n


def big_blanks(durations, blank=0, columns=None):
    """(columns, durations) as tuples of ints, checked as include/rnnt_mblank.h asks (all but `column < A`, which needs the
    logits).  columns=None: NeMo's layout, big blank i in column blank - 1 - i."""
    d = tuple(int(v) for v in durations)
    blank = int(blank)
    if len(d) > 8:
        raise ValueError("at most 8 big blanks, got %d" % len(d))
    if any(not 2 <= v <= 64 for v in d) or any(b <= a for a, b in zip(d, d[1:])):
        raise ValueError("big-blank durations must be strictly increasing and inside [2, 64]: %s" % (d,))
    if blank < 0:
        raise ValueError("blank = %d is not a column" % blank)
    if columns is None:
        if blank < len(d):
            raise ValueError("blank = %d leaves no room for %d big blanks in columns blank - 1 - i; pass big_blank_columns"
                             % (blank, len(d)))
        c = tuple(blank - 1 - i for i in range(len(d)))
    else:
        c = tuple(int(v) for v in columns)
    if len(c) != len(d):
        raise ValueError("%d big-blank columns for %d durations" % (len(c), len(d)))
    if any(v < 0 for v in c) or blank in c or len(set(c)) != len(c):
        raise ValueError("big-blank columns must be distinct, non-negative and different from blank = %d: %s" % (blank, c))
    return c, d


def _array(values):
    return (C.c_int * max(len(values), 1))(*values)


def _options(dev, blank, T, U):
    return _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream,
                            blank_label=int(blank), maxT=int(T), maxU=int(U), batch_first=True)


def _certify(logits, labels, act_lens, label_lens, cols, blank, validate):
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
        raise ValueError("the multi-blank loss runs on the GPU only: logits are on %s" % logits.device)
    if logits.dtype not in _DT:
        raise TypeError("logits must be torch.float32, float64, bfloat16 or float16")
    B, T, U, A = logits.shape
    if act_lens.shape[0] != B or label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a length per example.")
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    if any(c >= A for c in cols):
        raise ValueError("big-blank columns %s are not all columns (A = %d)" % (cols, A))
    check_gpu_arguments(logits, labels, act_lens, label_lens)
    if validate:
        max_t, max_l = torch.stack((act_lens, label_lens)).amax(1).tolist()
        if T != max_t:
            raise ValueError("Input length mismatch")
        if labels.shape[1] != max_l:
            raise ValueError("Output length mismatch")
        if labels.numel():
            inside = torch.arange(labels.shape[1], device=labels.device) < label_lens.unsqueeze(1)
            special = torch.tensor((int(blank),) + tuple(cols), dtype=labels.dtype, device=labels.device)
            if bool((torch.isin(labels, special) & inside).any()):
                raise ValueError("a label equals blank = %d or a big-blank column %s" % (int(blank), cols))


class _MultiBlank(Function):
    """Two-phase (compute_mblank_loss_fwd / _bwd): the forward call leaves the workspace, the backward call streams the
    gradient once with grad_output and the 1/N of 'mean' folded into its per-sample scale."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, cols, durs, blank, sigma, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, cols, blank, validate)
        K = len(durs)
        carr, darr = _array(cols), _array(durs)
        B, T, U, A = logits.shape
        dev = logits.device
        need_grad = logits.requires_grad
        cdt = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            costs = torch.empty(B, dtype=cdt, device=dev)
            ws = torch.empty(workspace_bytes(T, U, B, K, _DT[logits.dtype]), dtype=torch.uint8, device=dev)
            lab_ptr = labels.data_ptr() if labels.numel() else costs.data_ptr()    # maxU == 1: never read
            st = lib().compute_mblank_loss_fwd(logits.data_ptr(), carr, darr, K, float(sigma), lab_ptr,
                                               label_lens.data_ptr(), act_lens.data_ptr(), A, B, costs.data_ptr(),
                                               ws.data_ptr(), _options(dev, blank, T, U), _DT[logits.dtype],
                                               1 if need_grad else 0)
            _lib.check(st, "compute_mblank_loss_fwd")
        ctx.save_for_backward(logits)
        ctx.workspace = ws if need_grad else None
        ctx.carr, ctx.darr, ctx.K, ctx.blank = carr, darr, K, int(blank)
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
            st = lib().compute_mblank_loss_bwd(logits.data_ptr(), grads.data_ptr(), scale.data_ptr(), ctx.carr, ctx.darr,
                                               ctx.K, A, B, ctx.workspace.data_ptr(), _options(dev, ctx.blank, T, U),
                                               _DT[logits.dtype])
            _lib.check(st, "compute_mblank_loss_bwd")
            ctx.workspace.record_stream(torch.cuda.current_stream(dev))
        return grads, None, None, None, None, None, None, None, None, None


def rnnt_loss_mblank(acts, labels, act_lens, label_lens, big_blank_durations, blank=0, big_blank_columns=None, sigma=0.0,
                     reduction="mean", validate=True):
    """Multi-blank loss of raw logits (N, T, U, A) with one softmax over all A columns: the standard blank in column
    `blank` (one frame), big blank i in column big_blank_columns[i] (big_blank_durations[i] frames; 0 to 8 durations,
    strictly increasing, inside [2, 64]).  big_blank_columns=None: NeMo's layout, column blank - 1 - i (needs blank >= K).
    sigma: the logit under-normalisation (natural log).  labels (N, U - 1), act_lens, label_lens (N,) int32 on the device of
    the logits; no label may equal the blank or a big-blank column.  Costs float32 (float64 for float64 logits); reduction
    'none' | 'sum' | 'mean' as `rnnt_loss`.  validate=False skips the checks that read lengths and labels back: the call
    then only enqueues."""
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("reduction must be 'none', 'sum' or 'mean'")
    cols, durs = big_blanks(big_blank_durations, blank, big_blank_columns)
    return _MultiBlank.apply(acts, labels, act_lens, label_lens, cols, durs, int(blank), float(sigma), reduction, validate)


class MultiBlankLoss(Module):
    """Module form of `rnnt_loss_mblank`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, big_blank_durations, blank=0, big_blank_columns=None, sigma=0.0, reduction="mean"):
        super().__init__()
        if reduction not in ("none", "sum", "mean"):
            raise ValueError("reduction must be 'none', 'sum' or 'mean'")
        self.columns, self.durations = big_blanks(big_blank_durations, blank, big_blank_columns)
        self.blank, self.sigma, self.reduction = int(blank), float(sigma), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_mblank(acts, labels, act_lens, label_lens, self.durations, self.blank, self.columns, self.sigma,
                                self.reduction)
