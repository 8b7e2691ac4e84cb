"""The best path (Viterbi alignment) of the transducer lattice over edge log-probabilities the caller built, over
libwarprnnt_bestpath.so (include/rnnt_bestpath.h): the max-plus twin of `mi.mutual_information_recursion`.  px (B, S, T + 1)
-- or (B, S, T), the "modified" type whose symbol edges consume a frame -- and py (B, S + 1, T) hold the weights of the
lattice's edges; the score is the log weight of the best path (k2's sign), frames[b, s] the frame of its s-th symbol edge and
the gradient of the score the 0/1 indicator of its edges.  The recipe:

    px, py = get_rnnt_logprobs_pruned(logits, symbols, ranges, blank, boundary)      # warprnnt_pytorch.logprobs
    scores, frames = best_path(px, py, boundary)
    windows = alignment_windows(frames, ...)                                          # warprnnt_pytorch.ar

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib, _side
from .mi import _certify

__all__ = ["best_path", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "compute_rnnt_bestpath": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P,
                                        _lib.rnntOptions, C.c_int]),
    "compute_rnnt_bestpath_edges": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                              _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_bestpath.so", "best_path", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def back_words(T):
    """64-bit words of a row of `back`: ceil((T + 1) / 64)."""
    return (T + 64) // 64


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class _BestPath(Function):
    """forward: compute_rnnt_bestpath (with return_edges the indicators at once); backward: compute_rnnt_bestpath_edges with
    grad_output as the scale, or -- return_edges -- the indicators times grad_output, no launch of the library."""

    @staticmethod
    def forward(ctx, px, py, boundary, return_edges, validate):
        try:
            B, S, T, modified = _certify(px, py, boundary, validate)
        except ValueError as e:
            raise ValueError(str(e).replace("mutual_information_recursion", "best_path")) from None
        code, dev = _DT[px.dtype], px.device
        ctx.dims, ctx.code, ctx.edges = (B, S, T, modified), code, return_edges
        with torch.cuda.device(dev):
            opt = _side.options(dev, 0, T, S + 1)
            scores = torch.empty(B, dtype=torch.float64, device=dev)
            frames = torch.empty((B, S), dtype=torch.int32, device=dev)
            back = torch.empty((B, S + 1, back_words(T)), dtype=torch.int64, device=dev)
            ex = torch.empty_like(px) if return_edges else None
            ey = torch.empty_like(py) if return_edges else None
            _lib.check(lib().compute_rnnt_bestpath(_ptr(px), py.data_ptr(), _ptr(boundary), S, T, B, int(modified),
                                                   scores.data_ptr(), _ptr(frames), back.data_ptr(), _ptr(ex),
                                                   None if ey is None else ey.data_ptr(), opt, code),
                       "compute_rnnt_bestpath")
        ctx.mark_non_differentiable(frames, back)
        if return_edges:
            ctx.save_for_backward(ex, ey)
            ctx.mark_non_differentiable(ex, ey)
            return scores, frames, back, ex, ey
        ctx.save_for_backward(frames, scores, boundary)
        ctx.like = (px.shape, py.shape, px.dtype)
        return scores, frames, back

    @staticmethod
    def backward(ctx, grad_scores, *unused):
        B, S, T, modified = ctx.dims
        if ctx.edges:
            ex, ey = ctx.saved_tensors
            go = grad_scores.reshape(B, 1, 1)
            return (ex * go).to(ex.dtype), (ey * go).to(ey.dtype), None, None, None
        frames, scores, boundary = ctx.saved_tensors
        dev = grad_scores.device
        xs, ys, dtype = ctx.like
        with torch.cuda.device(dev):
            scale = grad_scores.reshape(-1).to(dtype=torch.float64).expand(B).contiguous()
            ex, ey = torch.empty(xs, dtype=dtype, device=dev), torch.empty(ys, dtype=dtype, device=dev)
            _lib.check(lib().compute_rnnt_bestpath_edges(_ptr(frames), scores.data_ptr(), _ptr(boundary), scale.data_ptr(), S, T,
                                                         B, int(modified), _ptr(ex), ey.data_ptr(),
                                                         _side.options(dev, 0, T, S + 1), ctx.code),
                       "compute_rnnt_bestpath_edges")
        return ex, ey, None, None, None


def best_path(px, py, boundary=None, return_edges=False, return_back=False, validate=True):
    """The best path of every sample's lattice.  px (B, S, T + 1) -- regular -- or (B, S, T) -- modified --, py (B, S + 1, T):
    edge log-probabilities (natural logs; -inf = no edge) of one floating dtype, contiguous, on one GPU; boundary: None or
    int64 (B, 4) rows [s0, t0, s1, t1] on that GPU.  Returns (scores, frames[, (px_path, py_path)][, back]): scores (B,)
    float64, the log weight of the best path, differentiable in px and py; frames (B, S) int32, for s0 <= s < s1 the t of the
    path's edge px[b, s, t] and -1 elsewhere (on exact ties every symbol as early as possible); with return_edges=True the
    0/1 indicators of the path's edges, made once in the forward call and multiplied by grad_output in backward; with
    return_back=True the back-pointer bits (B, S + 1, ceil((T + 1) / 64)) int64.  A sample without a path scores -inf, has
    frames -1 and a zero gradient.  validate=False skips the one check that reads device memory (the boundary's values): the
    call then only enqueues."""
    out = _BestPath.apply(px, py, boundary, bool(return_edges), validate)
    res = (out[0], out[1])
    if return_edges:
        res += ((out[3], out[4]),)
    if return_back:
        res += (out[2],)
    return res
