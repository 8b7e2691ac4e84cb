"""Alignment-restricted RNN-T loss (Mahadeokar et al., "Alignment Restricted Streaming Recurrent Neural Network Transducer",
SLT 2021) over libwarprnnt_ar.so (include/rnnt_ar.h).

The lattice is `rnnt_loss`'s, but label u of a sample may be emitted only at frames emit_lo[b, u] <= t <= emit_hi[b, u],
typically a few frames around a forced alignment: the standard way to bound a streaming model's emission delay.  Only the
band of rows a path can pass through is read.  The recipe:

    _, frames = rnnt_align(teacher_logits, labels, act_lens, label_lens)      # or any forced alignment, int32 (N, U - 1)
    emit_lo, emit_hi = alignment_windows(frames, left=0, right=5)
    loss = AlignmentRestrictedRNNTLoss(blank=0)(logits, labels, act_lens, label_lens, emit_lo, emit_hi)

Windows that reach past [0, T_b - 1] simply intersect with it; lo <= 0 and hi >= T_b - 1 leave a label unrestricted.

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side
from ._checks import check_contiguous, check_type

__all__ = ["rnnt_loss_ar", "AlignmentRestrictedRNNTLoss", "alignment_windows", "check_windows", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_ar": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_loss_ar": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int]),
    "compute_rnnt_loss_ar_fwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int,
                                           C.c_int]),
    "compute_rnnt_loss_ar_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_ar.so", "the alignment-restricted loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_ar", maxT, maxU, minibatch, dtype_code)


def alignment_windows(frames, left, right):
    """(emit_lo, emit_hi) = (frames - left, frames + right), int32 on the device of `frames`: label u may be emitted from
    `left` frames before its aligned frame to `right` frames behind it.  frames: int32 (N, U - 1), what `rnnt_align` returns;
    left, right: ints or per-label tensors that broadcast against it.  The -1 entries behind a sample's labels are passed
    through (they are never looked at)."""
    def spread(v):
        return v.to(device=frames.device) if torch.is_tensor(v) else int(v)
    behind = frames < 0
    lo = torch.where(behind, frames, frames - spread(left)).to(torch.int32)
    hi = torch.where(behind, frames, frames + spread(right)).to(torch.int32)
    return lo.contiguous(), hi.contiguous()


def check_windows(act_lens, label_lens, emit_lo, emit_hi):
    """Every sample has an alignment inside its windows: with e the prefix maximum of emit_lo (from 0) and l the suffix
    minimum of emit_hi (from T_b - 1), e_{u+1} <= l_u for every label u (include/rnnt_ar.h).  Host arithmetic on copies of
    the four tensors (one transfer for the lengths, one for the windows, when they are on a device)."""
    if emit_lo.numel() == 0:
        return
    tl, ll = torch.stack((act_lens, label_lens)).cpu().long()
    lo, hi = torch.stack((emit_lo, emit_hi)).cpu().long()
    behind = torch.arange(lo.shape[1])[None, :] >= ll[:, None]            # entries at u >= L_b: never looked at
    big = 1 << 40
    e = lo.masked_fill(behind, -big).cummax(1).values.clamp(min=0)        # e_{u+1}
    low = hi.masked_fill(behind, big).flip(1).cummin(1).values.flip(1)    # min(hi_u .. hi_{L_b - 1})
    low = torch.minimum(low, (tl - 1)[:, None])                            # l_u
    bad = (e > low) & ~behind
    if bad.any():
        b = int(bad.any(1).nonzero()[0])
        u = int(bad[b].nonzero()[0])
        raise ValueError("sample %d has no path: label %d needs a frame in [%d, %d]" % (b, u, int(e[b, u]), int(low[b, u])))


def _certify(logits, labels, act_lens, label_lens, emit_lo, emit_hi, blank, validate):
    for var, name in ((emit_lo, "emit_lo"), (emit_hi, "emit_hi")):
        check_type(var, torch.int32, name)
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  "the alignment-restricted loss runs on the GPU only: logits are on %(device)s")
    U, A = logits.shape[2], logits.shape[3]
    if U != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))
    for var, name in ((emit_lo, "emit_lo"), (emit_hi, "emit_hi")):
        check_contiguous(var, name)
        if var.shape != labels.shape:
            raise ValueError("%s must have the shape of labels" % name)
        if var.device != logits.device:
            raise ValueError("%s must be on the device of the logits" % name)
    if validate:
        check_windows(act_lens, label_lens, emit_lo, emit_hi)


class _AlignmentRestricted(Function):
    """Two-phase (compute_rnnt_loss_ar_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, emit_lo, emit_hi, blank, reduction, validate):
        _certify(logits, labels, act_lens, label_lens, emit_lo, emit_hi, blank, validate)
        B, T, U, A = logits.shape
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            lo_ptr, hi_ptr = (emit_lo.data_ptr(), emit_hi.data_ptr()) if emit_lo.numel() else (lab_ptr, lab_ptr)
            return lib().compute_rnnt_loss_ar_fwd(logits.data_ptr(), lab_ptr, label_lens.data_ptr(), act_lens.data_ptr(),
                                                  lo_ptr, hi_ptr, A, B, costs, ws,
                                                  _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.blank = int(blank)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, code), reduction, call,
                             "compute_rnnt_loss_ar_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_rnnt_loss_ar_bwd(logits.data_ptr(), grads, scale, A, B, ws,
                                                  _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_rnnt_loss_ar_bwd")
        return grads, None, None, None, None, None, None, None, None


def rnnt_loss_ar(acts, labels, act_lens, label_lens, emit_lo, emit_hi, blank=0, reduction="mean", validate=True):
    """Alignment-restricted RNN-T loss of raw logits (N, T, U, A) with one softmax over all A columns, blank in column
    `blank` (any column).  labels (N, U - 1), act_lens, label_lens (N,) int32 on the device of the logits; emit_lo, emit_hi
    int32 (N, U - 1) on the same device: the inclusive first and last frame at which label u may be emitted
    (`alignment_windows`).  Costs float32 (float64 for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.
    validate=True reads the lengths and the windows back and raises ValueError for a sample whose windows leave no alignment;
    validate=False skips every check that reads device memory: the call then only enqueues, and such a sample costs +inf."""
    _side.check_reduction(reduction)
    return _AlignmentRestricted.apply(acts, labels, act_lens, label_lens, emit_lo, emit_hi, blank, reduction, validate)


class AlignmentRestrictedRNNTLoss(Module):
    """Module form of `rnnt_loss_ar`: forward(acts, labels, act_lens, label_lens, emit_lo, emit_hi)."""

    def __init__(self, blank=0, reduction="mean"):
        super().__init__()
        _side.check_reduction(reduction)
        self.blank, self.reduction = int(blank), reduction

    def forward(self, acts, labels, act_lens, label_lens, emit_lo, emit_hi):
        return rnnt_loss_ar(acts, labels, act_lens, label_lens, emit_lo, emit_hi, self.blank, self.reduction)
