"""Prune ranges from the occupations of a lattice the caller built, and the posterior mass a set of windows keeps, over
libwarprnnt_ranges.so (include/rnnt_ranges.h).  `mi.mutual_information_recursion(..., return_grad=True)` returns the
occupations px_grad / py_grad of any px / py lattice -- smoothed, delay-penalised, HAT-style, internal-LM-subtracted, regular or
modified; `RNNTLossPruned`, `PrunedStreamingRNNTLoss`, `joiner_pruned` and `logprobs` consume `ranges` int32 (B, T).  This
module is the step between the two (INTEGRATION.md sections 16 and 23):

    scores, (px_grad, py_grad) = mutual_information_recursion(px, py, boundary, return_grad=True)
    ranges = prune_ranges_from_occupations(px_grad, py_grad, boundary, s_range=5)            # int32 (B, T)
    kept = range_coverage(px_grad, py_grad, ranges, 5, boundary)                            # float64 (B, T)

The occupations must be the UNSCALED ones, as `return_grad=True` hands them out: gradients that carry a negative
grad_output turn the argmax round.  The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch

from . import _lib, _side

__all__ = ["prune_ranges_from_occupations", "get_rnnt_prune_ranges", "range_coverage", "library_path"]

_DT, _P = _side.DT, _side.P
_I = C.c_int
EXPORTS = {
    "compute_rnnt_prune_ranges_occ": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _lib.rnntOptions, _I]),
    "compute_rnnt_range_coverage": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _lib.rnntOptions, _I]),
}
_LIB = _side.Library("libwarprnnt_ranges.so", "prune_ranges_from_occupations", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _dims(px_grad, py_grad):
    """-> (B, S, T, modified) from the shapes alone: py_grad (B, S + 1, T), px_grad (B, S, T + 1) or (B, S, T)."""
    for t, name in ((px_grad, "px_grad"), (py_grad, "py_grad")):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
        if t.dim() != 3:
            raise ValueError("%s must be a 3D tensor" % name)
    B, S1, T = py_grad.shape
    S = S1 - 1
    if S < 0 or T < 1 or B < 1:
        raise ValueError("py_grad must be (B, S + 1, T) with B >= 1, S >= 0 and T >= 1")
    if px_grad.shape[0] != B or px_grad.shape[1] != S or px_grad.shape[2] not in (T, T + 1):
        raise ValueError("px_grad must be (B, S, T + 1) or (B, S, T) for py_grad (B, S + 1, T): got px_grad %s, py_grad %s"
                         % (tuple(px_grad.shape), tuple(py_grad.shape)))
    return B, S, T, px_grad.shape[2] == T


def _certify(px_grad, py_grad, boundary, what):
    if px_grad.dtype not in _DT or py_grad.dtype != px_grad.dtype:
        raise TypeError("px_grad and py_grad must share one dtype of torch.float32, float64, bfloat16, float16")
    if not px_grad.is_contiguous() or not py_grad.is_contiguous():
        raise ValueError("px_grad and py_grad must be contiguous")
    if boundary is not None:
        if not torch.is_tensor(boundary) or boundary.dtype != torch.int64 or tuple(boundary.shape) != (py_grad.shape[0], 4):
            raise ValueError("boundary must be an int64 tensor of shape (B, 4)")
        if not boundary.is_contiguous():
            raise ValueError("boundary must be contiguous")
    if not px_grad.is_cuda or not py_grad.is_cuda:
        raise ValueError("%s runs on the GPU only: px_grad is on %s, py_grad on %s" % (what, px_grad.device, py_grad.device))
    if px_grad.device != py_grad.device or (boundary is not None and boundary.device != px_grad.device):
        raise ValueError("px_grad, py_grad and boundary must be on one device")


def _width(s_range, S):
    if not isinstance(s_range, int) or isinstance(s_range, bool) or s_range < 1:
        raise ValueError("s_range must be an int >= 1: got %r" % (s_range,))
    return S + 1 if s_range > S else s_range              # as k2: a window wider than the symbols is the whole column


def prune_ranges_from_occupations(px_grad, py_grad, boundary=None, s_range=5, step=None, validate=True):
    """Window starts int32 (B, T), on the inputs' device, from the occupations px_grad (B, S, T + 1) -- regular -- or
    (B, S, T) -- modified -- and py_grad (B, S + 1, T) of `mutual_information_recursion(..., return_grad=True)`: per frame
    the start of the s_range rows that hold the most occupancy (ties: the smallest start), repaired so that the starts
    begin at 0, never decrease, advance by at most `step` per frame and end at S_b + 1 - s_range -- a path through the
    windows is guaranteed where one fits (include/rnnt_ranges.h has the rule in full).  boundary: None or int64 (B, 4), of
    which columns 2 and 3 (S_b, T_b) are read; frames t >= T_b get 0.  s_range > S becomes S + 1.  step=None: max(1,
    s_range - 1) for the regular type and 1 for the modified type, whose symbol edges consume a frame (k2's slopes).  There
    is no gradient.  The call is enqueued on the current stream.  validate=False skips the argument checks: it only
    enqueues."""
    B, S, T, modified = _dims(px_grad, py_grad)
    if validate:
        _certify(px_grad, py_grad, boundary, "prune_ranges_from_occupations")
    R = _width(s_range, S)
    if step is None:
        step = 1 if modified else max(1, R - 1)
    if validate and (not isinstance(step, int) or isinstance(step, bool) or not 1 <= step <= max(1, R - 1)):
        raise ValueError("step must be an int in [1, max(1, s_range - 1)] = [1, %d]: got %r" % (max(1, R - 1), step))
    dev = py_grad.device
    with torch.no_grad(), torch.cuda.device(dev):
        ranges = torch.empty((B, T), dtype=torch.int32, device=dev)
        _lib.check(lib().compute_rnnt_prune_ranges_occ(_ptr(px_grad), py_grad.data_ptr(), _ptr(boundary), S, T, B,
                                                       int(modified), R, int(step), ranges.data_ptr(),
                                                       _side.options(dev, 0, T, S + 1), _DT[py_grad.dtype]),
                   "compute_rnnt_prune_ranges_occ")
    return ranges


def get_rnnt_prune_ranges(px_grad, py_grad, boundary, s_range):
    """k2's call and return shape: int64 (B, T, s_range), `starts[..., None] + arange(s_range)`, the starts those of
    `prune_ranges_from_occupations` with its default step.  The RULE is this library's, not k2's: a path through the windows
    is guaranteed, and ties go to the smallest start.  It differs from k2's at padding frames (start 0 here) and near ties;
    no parity with k2 is claimed."""
    _, S, _, _ = _dims(px_grad, py_grad)
    starts = prune_ranges_from_occupations(px_grad, py_grad, boundary, s_range)
    R = _width(s_range, S)
    return starts.to(torch.int64).unsqueeze(-1) + torch.arange(R, dtype=torch.int64, device=starts.device)


def range_coverage(px_grad, py_grad, ranges, s_range, boundary=None, validate=True):
    """float64 (B, T): the share of frame t's occupancy that lies in the rows [ranges[b, t], ranges[b, t] + s_range) -- the
    posterior mass the windows keep, the figure to look at when choosing s_range.  ranges int32 (B, T) from anywhere
    (`prune_ranges_from_occupations`, `prune_ranges` on the additive joint, hand-made); a start outside [0, S_b] is clamped.
    0 for frames t >= T_b and for columns without occupancy.  The sums are fp64 in a fixed order: two calls give the same
    bits."""
    B, S, T, modified = _dims(px_grad, py_grad)
    if validate:
        _certify(px_grad, py_grad, boundary, "range_coverage")
        if not torch.is_tensor(ranges) or ranges.dtype != torch.int32 or tuple(ranges.shape) != (B, T):
            raise ValueError("ranges must be an int32 tensor of shape (B, T) = %s" % ((B, T),))
        if not ranges.is_contiguous():
            raise ValueError("ranges must be contiguous")
        if ranges.device != py_grad.device:
            raise ValueError("ranges must be on the device of px_grad and py_grad: it is on %s" % ranges.device)
    R = _width(s_range, S)
    dev = py_grad.device
    with torch.no_grad(), torch.cuda.device(dev):
        kept = torch.empty((B, T), dtype=torch.float64, device=dev)
        _lib.check(lib().compute_rnnt_range_coverage(_ptr(px_grad), py_grad.data_ptr(), _ptr(boundary), ranges.data_ptr(), S,
                                                     T, B, int(modified), R, kept.data_ptr(),
                                                     _side.options(dev, 0, T, S + 1), _DT[py_grad.dtype]),
                   "compute_rnnt_range_coverage")
    return kept
