"""The expected cost of a path of the transducer lattice, and the entropy of its alignment posterior, over edge
log-probabilities the caller built, over libwarprnnt_expect.so (include/rnnt_expect.h): the expectation semiring on the lattice
of `mi.mutual_information_recursion`.  px (B, S, T + 1) -- or (B, S, T), the "modified" type whose symbol edges consume a
frame -- and py (B, S + 1, T) hold the weights of the lattice's edges, cx and cy an additive cost of each edge; the result is
E[sum of the costs along a path] under p(path) ~ exp(weight of the path), differentiable in all four tensors (the gradient in
the weights is a covariance: no number of calls of `mi` yields it).  The recipes:

    px, py = get_rnnt_logprobs_joint(logits, symbols, blank, boundary)               # warprnnt_pytorch.logprobs
    cx = torch.arange(T + 1.0, device=px.device).expand_as(px).contiguous()          # the cost of a symbol edge: its frame
    latency = expected_cost(px, py, cx, torch.zeros_like(py), boundary)              # minimum expected latency
    entropy = alignment_entropy(px, py, boundary)                                    # H = log Z - E[W]

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib, _side
from .mi import _certify

__all__ = ["expected_cost", "alignment_entropy", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "compute_rnnt_expect": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                      _lib.rnntOptions, C.c_int]),
    "compute_rnnt_expect_fwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P,
                                          _lib.rnntOptions, C.c_int]),
    "compute_rnnt_expect_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _P, _P, _P, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_expect.so", "expected_cost", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _certify_costs(px, py, cx, cy):
    """cx / cy against px / py: a tensor of the weight's shape, dtype, device and layout."""
    for c, w, name in ((cx, px, "x"), (cy, py, "y")):
        if not torch.is_tensor(c) or c.shape != w.shape or c.dtype != w.dtype:
            raise ValueError("c%s must have the shape and dtype of p%s: got %s, p%s %s %s"
                             % (name, name, (tuple(c.shape), c.dtype) if torch.is_tensor(c) else type(c), name,
                                tuple(w.shape), w.dtype))
        if not c.is_contiguous():
            raise ValueError("cx and cy must be contiguous")
        if c.device != w.device:
            raise ValueError("cx and cy must be on the device of px and py: c%s is on %s" % (name, c.device))


class _Expect(Function):
    """Two-phase: compute_rnnt_expect_fwd leaves `nodes`; compute_rnnt_expect_bwd takes the two incoming gradients as its
    per-sample scales and skips the cost gradients when neither cost needs one."""

    @staticmethod
    def forward(ctx, px, py, cx, cy, boundary, validate):
        try:
            B, S, T, modified = _certify(px, py, boundary, validate)
        except ValueError as e:
            raise ValueError(str(e).replace("mutual_information_recursion", "expected_cost")) from None
        _certify_costs(px, py, cx, cy)
        code, dev = _DT[px.dtype], px.device
        ctx.dims, ctx.code = (B, S, T, modified), code
        with torch.cuda.device(dev):
            scores = torch.empty(B, dtype=torch.float64, device=dev)
            expect = torch.empty(B, dtype=torch.float64, device=dev)
            nodes = torch.empty((B, S + 1, T + 1, 2), dtype=torch.float64, device=dev)
            _lib.check(lib().compute_rnnt_expect_fwd(_ptr(px), py.data_ptr(), _ptr(cx), cy.data_ptr(), _ptr(boundary), S, T, B,
                                                     int(modified), scores.data_ptr(), expect.data_ptr(), nodes.data_ptr(),
                                                     _side.options(dev, 0, T, S + 1), code),
                       "compute_rnnt_expect_fwd")
        ctx.save_for_backward(px, py, cx, cy, boundary, nodes, scores, expect)
        ctx.mark_non_differentiable(nodes)
        return expect, scores, nodes

    @staticmethod
    def backward(ctx, g_expect, g_scores, *unused):
        B, S, T, modified = ctx.dims
        px, py, cx, cy, boundary, nodes, scores, expect = ctx.saved_tensors
        dev = px.device
        costs = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        with torch.cuda.device(dev):
            ge = g_expect.reshape(-1).to(dtype=torch.float64).expand(B).contiguous()
            gs = g_scores.reshape(-1).to(dtype=torch.float64).expand(B).contiguous()
            gx, gy = torch.empty_like(px), torch.empty_like(py)
            hx, hy = (torch.empty_like(px), torch.empty_like(py)) if costs else (None, None)
            _lib.check(lib().compute_rnnt_expect_bwd(_ptr(px), py.data_ptr(), _ptr(cx), cy.data_ptr(), _ptr(boundary),
                                                     nodes.data_ptr(), scores.data_ptr(), expect.data_ptr(), ge.data_ptr(),
                                                     gs.data_ptr(), S, T, B, int(modified), _ptr(gx), gy.data_ptr(),
                                                     _ptr(hx), None if hy is None else hy.data_ptr(),
                                                     _side.options(dev, 0, T, S + 1), ctx.code),
                       "compute_rnnt_expect_bwd")
        return gx, gy, hx, hy, None, None


def expected_cost(px, py, cx, cy, boundary=None, return_scores=False, validate=True):
    """E[sum of the costs along a path] of every sample's lattice.  px (B, S, T + 1) -- regular -- or (B, S, T) -- modified
    --, py (B, S + 1, T): edge log-probabilities (natural logs; -inf = no edge) of one floating dtype, contiguous, on one GPU;
    cx, cy: the additive cost of each edge, shaped, typed and placed as px, py (a cost on a -inf edge is never looked at, so
    cx = px, cy = py is legal); boundary: None or int64 (B, 4) rows [s0, t0, s1, t1] on that GPU.  Returns expect (B,)
    float64, or with return_scores=True (expect, scores): scores (B,) float64 is log Z, `mutual_information_recursion`'s.
    Both are differentiable in all four tensors.  A sample without a path has expect 0, scores -inf and zero gradients.
    validate=False skips the one check that reads device memory (the boundary's values): the call then only enqueues."""
    expect, scores, _ = _Expect.apply(px, py, cx, cy, boundary, validate)
    return (expect, scores) if return_scores else expect


def alignment_entropy(px, py, boundary=None, validate=True):
    """The entropy (B,) float64 of the posterior over the paths of every sample's lattice, H = log Z - E[W]: the expected
    cost with the weights as their own costs.  One forward and one backward call; differentiable in px and py."""
    expect, scores, _ = _Expect.apply(px, py, px, py, boundary, validate)
    return scores - expect
