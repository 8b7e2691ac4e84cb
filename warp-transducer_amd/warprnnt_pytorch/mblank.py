"""Multi-blank transducer loss (Xu et al., "Multi-blank Transducers for Speech Recognition", ICASSP 2023; NeMo's
MultiblankRNNTLoss) over libwarprnnt_mblank.so (include/rnnt_mblank.h).

Besides the standard blank (one frame) the vocabulary holds K "big blank" columns, each of which consumes a fixed number of
frames.  The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A) raw logits, one softmax over all A columns
    loss = MultiBlankLoss(big_blank_durations=[2, 4, 8], blank=A - 1, sigma=0.05)(logits, labels, act_lens, label_lens)

With `big_blank_columns=None` the columns are NeMo's: big blank i sits in column `blank - 1 - i`.

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side

__all__ = ["rnnt_loss_mblank", "MultiBlankLoss", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_mblank": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_mblank_loss": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                      _lib.rnntOptions, C.c_int]),
    "compute_mblank_loss_fwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                          _lib.rnntOptions, C.c_int, C.c_int]),
    "compute_mblank_loss_bwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_mblank.so", "the multi-blank loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, num_big_blanks, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_mblank", maxT, maxU, minibatch, num_big_blanks, dtype_code)


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


def _certify(logits, labels, act_lens, label_lens, cols, blank, validate):
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  "the multi-blank loss runs on the GPU only: logits are on %(device)s")
    U, A = logits.shape[2], logits.shape[3]
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    if any(c >= A for c in cols):
        raise ValueError("big-blank columns %s are not all columns (A = %d)" % (cols, A))
    if validate and labels.numel():
        inside = torch.arange(labels.shape[1], device=labels.device) < label_lens.unsqueeze(1)
        special = torch.tensor((int(blank),) + tuple(cols), dtype=labels.dtype, device=labels.device)
        if bool((torch.isin(labels, special) & inside).any()):
            raise ValueError("a label equals blank = %d or a big-blank column %s" % (int(blank), cols))


class _MultiBlank(Function):
    """Two-phase (compute_mblank_loss_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, cols, durs, blank, sigma, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, cols, blank, validate)
        K = len(durs)
        carr, darr = _array(cols), _array(durs)
        B, T, U, A = logits.shape
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_mblank_loss_fwd(logits.data_ptr(), carr, darr, K, float(sigma), lab_ptr,
                                                 label_lens.data_ptr(), act_lens.data_ptr(), A, B, costs, ws,
                                                 _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.carr, ctx.darr, ctx.K, ctx.blank = carr, darr, K, int(blank)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, K, code), reduction, call,
                             "compute_mblank_loss_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_mblank_loss_bwd(logits.data_ptr(), grads, scale, ctx.carr, ctx.darr, ctx.K, A, B, ws,
                                                 _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_mblank_loss_bwd")
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
    _side.check_reduction(reduction)
    cols, durs = big_blanks(big_blank_durations, blank, big_blank_columns)
    return _MultiBlank.apply(acts, labels, act_lens, label_lens, cols, durs, int(blank), float(sigma), reduction, validate)


class MultiBlankLoss(Module):
    """Module form of `rnnt_loss_mblank`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, big_blank_durations, blank=0, big_blank_columns=None, sigma=0.0, reduction="mean"):
        super().__init__()
        _side.check_reduction(reduction)
        self.columns, self.durations = big_blanks(big_blank_durations, blank, big_blank_columns)
        self.blank, self.sigma, self.reduction = int(blank), float(sigma), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_mblank(acts, labels, act_lens, label_lens, self.durations, self.blank, self.columns, self.sigma,
                                self.reduction)
