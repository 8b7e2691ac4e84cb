"""The transducer lattice over edge log-probabilities the caller built: k2 / fast_rnnt's `mutual_information_recursion`, over
libwarprnnt_mi.so (include/rnnt_mi.h).  No logits, no softmax, no labels: px (B, S, T + 1) -- or (B, S, T), the "modified"
type whose symbol edges consume a frame -- and py (B, S + 1, T) hold the weights of the lattice's edges; the score is the
log of the total over the paths (k2's sign, not a cost) and its gradient the occupation of every edge.  The recipe
(INTEGRATION.md section 16):

    px, py = get_rnnt_logprobs_smoothed(lm, am, symbols, blank, lm_only_scale, am_only_scale, boundary)     # the user's torch
    scores, (px_grad, py_grad) = mutual_information_recursion(px, py, boundary, return_grad=True)
    simple_loss = -scores.sum()
    ranges = get_rnnt_prune_ranges(px_grad, py_grad, boundary, s_range)                                     # the user's torch

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib, _side

__all__ = ["mutual_information_recursion", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_mi": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_mi": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _lib.rnntOptions, C.c_int]),
    "compute_rnnt_mi_fwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int,
                                      C.c_int]),
    "compute_rnnt_mi_bwd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_mi.so", "mutual_information_recursion", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(S, T, minibatch, modified, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_mi", S, T, minibatch, int(bool(modified)), dtype_code)


def _certify(px, py, boundary, validate):
    """-> (B, S, T, modified).  Everything but the boundary's values is checked from the tensors' descriptions, shapes and
    dtypes before devices; validate: the one device-to-host read, 0 <= s0 <= s1 <= S and 0 <= t0 <= t1 <= T in every row."""
    for t, name in ((px, "px"), (py, "py")):
        if not torch.is_tensor(t) or t.dim() != 3:
            raise ValueError("%s must be a 3D tensor" % name)
    if px.dtype not in _DT or py.dtype != px.dtype:
        raise ValueError("px and py must share one dtype of torch.float32, float64, bfloat16, float16")
    B, S1, T = py.shape
    S = S1 - 1
    if S < 0 or T < 1 or B < 1:
        raise ValueError("py must be (B, S + 1, T) with B >= 1, S >= 0 and T >= 1")
    if px.shape[0] != B or px.shape[1] != S or px.shape[2] not in (T, T + 1):
        raise ValueError("px must be (B, S, T + 1) or (B, S, T) for py (B, S + 1, T): got px %s, py %s"
                         % (tuple(px.shape), tuple(py.shape)))
    if not px.is_contiguous() or not py.is_contiguous():
        raise ValueError("px and py must be contiguous")
    if boundary is not None:
        if not torch.is_tensor(boundary) or boundary.dtype != torch.int64 or tuple(boundary.shape) != (B, 4):
            raise ValueError("boundary must be an int64 tensor of shape (B, 4)")
        if not boundary.is_contiguous():
            raise ValueError("boundary must be contiguous")
    if not px.is_cuda or not py.is_cuda:
        raise ValueError("mutual_information_recursion runs on the GPU only: px is on %s, py on %s" % (px.device, py.device))
    if px.device != py.device or (boundary is not None and boundary.device != px.device):
        raise ValueError("px, py and boundary must be on one device")
    if boundary is not None and validate:
        s0, t0, s1, t1 = boundary.t().tolist()
        for b in range(B):
            if not (0 <= s0[b] <= s1[b] <= S and 0 <= t0[b] <= t1[b] <= T):
                raise ValueError("boundary[%d] = %s is outside 0 <= s0 <= s1 <= %d, 0 <= t0 <= t1 <= %d"
                                 % (b, [s0[b], t0[b], s1[b], t1[b]], S, T))
    return B, S, T, px.shape[2] == T


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _score_dtype(px):
    return torch.float64 if px.dtype == torch.float64 else torch.float32


class _MutualInformation(Function):
    """Two-phase (compute_rnnt_mi_fwd / _bwd).  return_grad: the forward call makes the occupations at once (the backward
    entry at scale 1) and hands them out; backward then multiplies them by grad_output and launches nothing."""

    @staticmethod
    def forward(ctx, px, py, boundary, return_grad, validate):
        B, S, T, modified = _certify(px, py, boundary, validate)
        code, dev = _DT[px.dtype], px.device
        need_grad = px.requires_grad or py.requires_grad
        ctx.dims, ctx.code, ctx.workspace = (B, S, T, modified), code, None
        with torch.cuda.device(dev):
            opt = _side.options(dev, 0, T, S + 1)
            scores = torch.empty(B, dtype=_score_dtype(px), device=dev)
            ws = torch.empty(workspace_bytes(S, T, B, modified, code), dtype=torch.uint8, device=dev)
            if return_grad:
                gx, gy = torch.empty_like(px), torch.empty_like(py)
                _lib.check(lib().compute_rnnt_mi(_ptr(px), py.data_ptr(), _ptr(boundary), S, T, B, int(modified),
                                                 scores.data_ptr(), _ptr(gx), gy.data_ptr(), ws.data_ptr(), opt, code),
                           "compute_rnnt_mi")
                ws.record_stream(torch.cuda.current_stream(dev))
                ctx.save_for_backward(gx, gy)
                ctx.mark_non_differentiable(gx, gy)
                return scores, gx, gy
            _lib.check(lib().compute_rnnt_mi_fwd(_ptr(px), py.data_ptr(), _ptr(boundary), S, T, B, int(modified),
                                                 scores.data_ptr(), ws.data_ptr(), opt, code, 1 if need_grad else 0),
                       "compute_rnnt_mi_fwd")
            if need_grad:
                ctx.workspace = ws
                ctx.like = (px.shape, py.shape, px.dtype)
            else:
                ws.record_stream(torch.cuda.current_stream(dev))
        return scores

    @staticmethod
    def backward(ctx, grad_scores, *unused):
        B, S, T, modified = ctx.dims
        if ctx.workspace is None:                          # return_grad: the occupations are there
            gx, gy = ctx.saved_tensors
            go = grad_scores.reshape(B, 1, 1)
            return (gx * go).to(gx.dtype), (gy * go).to(gy.dtype), None, None, None
        dev = grad_scores.device
        xs, ys, dtype = ctx.like
        with torch.cuda.device(dev):
            cdt = torch.float64 if dtype == torch.float64 else torch.float32
            scale = grad_scores.reshape(-1).to(dtype=cdt).expand(B).contiguous()
            gx, gy = torch.empty(xs, dtype=dtype, device=dev), torch.empty(ys, dtype=dtype, device=dev)
            _lib.check(lib().compute_rnnt_mi_bwd(_ptr(gx), gy.data_ptr(), scale.data_ptr(), S, T, B, int(modified),
                                                 ctx.workspace.data_ptr(), _side.options(dev, 0, T, S + 1), ctx.code),
                       "compute_rnnt_mi_bwd")
            ctx.workspace.record_stream(torch.cuda.current_stream(dev))
        return gx, gy, None, None, None


def mutual_information_recursion(px, py, boundary=None, return_grad=False, validate=True):
    """k2's `mutual_information_recursion`.  px (B, S, T + 1) -- regular -- or (B, S, T) -- modified --, py (B, S + 1, T): edge
    log-probabilities (natural logs; -inf = no edge) of one floating dtype, contiguous, on one GPU; boundary: None or int64
    (B, 4) rows [s0, t0, s1, t1] on that GPU.  Returns scores (B,) -- float32, float64 for float64 inputs --, or with
    return_grad=True (scores, (px_grad, py_grad)): the occupation of every edge, exact 0 outside a sample's rectangle.
    Differentiable in px and py; with return_grad=True the occupations are computed once and serve the backward pass too.
    A sample without a path scores -inf and has zero gradients.  validate=False skips the one check that reads device memory
    (the boundary's values): the call then only enqueues."""
    if return_grad:
        scores, gx, gy = _MutualInformation.apply(px, py, boundary, True, validate)
        return scores, (gx, gy)
    return _MutualInformation.apply(px, py, boundary, False, validate)
