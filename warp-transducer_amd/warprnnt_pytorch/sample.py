"""Alignments drawn from the posterior of the transducer lattice, and the weight of given alignments, over edge
log-probabilities the caller built, over libwarprnnt_sample.so (include/rnnt_sample.h).  px (B, S, T + 1) -- or (B, S, T), the
"modified" type whose symbol edges consume a frame -- and py (B, S + 1, T) hold the weights of the lattice's edges, as for
`mi.mutual_information_recursion`, `bestpath.best_path` and `expect.expected_cost`.  `sample_paths` draws K exact samples per
lattice from p(path) ~ exp W(path); `path_scores` is W of given paths, differentiable in px and py.  Objectives that are
not sums over edges get a score-function estimator in two lines:

    frames, logq, scores = sample_paths(px, py, 16, boundary, generator=g)
    loss = ((cost(frames) - baseline).detach()
            * (path_scores(px, py, frames, boundary) - mutual_information_recursion(px, py, boundary)[:, None])).mean()

The library holds no generator: the uniforms come from `torch.rand` with the caller's generator, or from the caller.  The
library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib, _side
from .mi import _certify

__all__ = ["sample_paths", "path_scores", "library_path"]

_DT, _P = _side.DT, _side.P
_I = C.c_int
EXPORTS = {
    "compute_rnnt_sample": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _lib.rnntOptions, _I]),
    "compute_rnnt_sample_walk": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _lib.rnntOptions, _I]),
    "compute_rnnt_path_weights": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _lib.rnntOptions, _I]),
    "compute_rnnt_path_edges": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _lib.rnntOptions, _I]),
}
_LIB = _side.Library("libwarprnnt_sample.so", "sample_paths", EXPORTS)
library_path, lib = _LIB.path, _LIB.load
MAX_SAMPLES = 1024


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _certified(px, py, boundary, validate, what):
    try:
        return _certify(px, py, boundary, validate)
    except ValueError as e:
        raise ValueError(str(e).replace("mutual_information_recursion", what)) from None


def _certify_samples(num_samples):
    if not isinstance(num_samples, int) or isinstance(num_samples, bool) or not 1 <= num_samples <= MAX_SAMPLES:
        raise ValueError("num_samples must be an int in [1, %d]: got %r" % (MAX_SAMPLES, num_samples))


def _certify_uniforms(uniforms, py, K):
    """uniforms against py (B, S + 1, T): float32 (B, K, S + T), contiguous, on py's device."""
    B, S1, T = py.shape
    want = (B, K, S1 - 1 + T)
    if not torch.is_tensor(uniforms) or uniforms.dtype != torch.float32 or tuple(uniforms.shape) != want:
        raise ValueError("uniforms must be a float32 tensor of shape (B, K, S + T) = %s: got %s"
                         % (want, (tuple(uniforms.shape), uniforms.dtype) if torch.is_tensor(uniforms) else type(uniforms)))
    if not uniforms.is_contiguous():
        raise ValueError("uniforms must be contiguous")
    if uniforms.device != py.device:
        raise ValueError("uniforms must be on the device of px and py: it is on %s" % uniforms.device)


def _certify_frames(frames, py):
    """-> frames as (B, K, S), K: an int32 tensor (B, K, S) or (B, S), contiguous, on py's device."""
    B, S1, _ = py.shape
    S = S1 - 1
    if not torch.is_tensor(frames) or frames.dtype != torch.int32 or frames.dim() not in (2, 3) or frames.shape[0] != B \
            or frames.shape[-1] != S:
        raise ValueError("frames must be an int32 tensor of shape (B, K, S) or (B, S) with B = %d, S = %d: got %s"
                         % (B, S, (tuple(frames.shape), frames.dtype) if torch.is_tensor(frames) else type(frames)))
    if frames.dim() == 2:
        frames = frames.unsqueeze(1)
    K = frames.shape[1]
    if not 1 <= K <= MAX_SAMPLES:
        raise ValueError("frames must hold between 1 and %d paths per sample: got %d" % (MAX_SAMPLES, K))
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous")
    if frames.device != py.device:
        raise ValueError("frames must be on the device of px and py: it is on %s" % frames.device)
    return frames, K


def sample_paths(px, py, num_samples, boundary=None, generator=None, uniforms=None, return_alpha=False, validate=True):
    """K = num_samples alignments per lattice, drawn exactly from p(path) ~ exp W(path).  px (B, S, T + 1) -- regular -- or
    (B, S, T) -- modified --, py (B, S + 1, T): edge log-probabilities (natural logs; -inf = no edge) of one floating dtype,
    contiguous, on one GPU; boundary: None or int64 (B, 4) rows [s0, t0, s1, t1] on that GPU.  The uniforms are
    torch.rand((B, K, S + T), generator=generator) on that GPU, or `uniforms` (float32, that shape, in [0, 1)) where given.
    Returns (frames (B, K, S) int32, logq (B, K) float64, scores (B,) float64) and with return_alpha=True also alpha
    (B, S + 1, T + 1) float64: frames in `best_path`'s convention (the t of every symbol edge, -1 outside [s0, s1)), logq =
    W(path) - scores the log-probability of each drawn path, scores = log Z.  A lattice without a path has frames -1 and logq
    NaN.  Takes no gradient (`path_scores` does).  validate=False skips the one check that reads device memory (the
    boundary's values): the call then only enqueues."""
    B, S, T, modified = _certified(px, py, boundary, validate, "sample_paths")
    _certify_samples(num_samples)
    K, dev = num_samples, px.device
    if uniforms is not None:
        _certify_uniforms(uniforms, py, K)
    with torch.no_grad(), torch.cuda.device(dev):
        if uniforms is None:
            uniforms = torch.rand((B, K, S + T), dtype=torch.float32, device=dev, generator=generator)
        scores = torch.empty(B, dtype=torch.float64, device=dev)
        alpha = torch.empty((B, S + 1, T + 1), dtype=torch.float64, device=dev)
        frames = torch.empty((B, K, S), dtype=torch.int32, device=dev)
        weights = torch.empty((B, K), dtype=torch.float64, device=dev)
        _lib.check(lib().compute_rnnt_sample(_ptr(px), py.data_ptr(), _ptr(boundary), _ptr(uniforms), S, T, B, K,
                                             int(modified), scores.data_ptr(), alpha.data_ptr(), _ptr(frames),
                                             weights.data_ptr(), _side.options(dev, 0, T, S + 1), _DT[px.dtype]),
                   "compute_rnnt_sample")
        logq = weights - scores[:, None]
    return (frames, logq, scores, alpha) if return_alpha else (frames, logq, scores)


class _PathScores(Function):
    """Forward: compute_rnnt_path_weights.  Backward: compute_rnnt_path_edges with coeff = grad_output."""

    @staticmethod
    def forward(ctx, px, py, frames, boundary, dims):
        B, S, T, modified, K = dims
        dev = px.device
        with torch.cuda.device(dev):
            weights = torch.empty((B, K), dtype=torch.float64, device=dev)
            _lib.check(lib().compute_rnnt_path_weights(_ptr(px), py.data_ptr(), _ptr(boundary), _ptr(frames), S, T, B, K,
                                                       int(modified), weights.data_ptr(), _side.options(dev, 0, T, S + 1),
                                                       _DT[px.dtype]),
                       "compute_rnnt_path_weights")
        ctx.save_for_backward(frames, boundary)
        ctx.dims, ctx.like = dims, (px.shape, py.shape, px.dtype, dev)
        return weights

    @staticmethod
    def backward(ctx, grad_output):
        B, S, T, modified, K = ctx.dims
        frames, boundary = ctx.saved_tensors
        xs, ys, dtype, dev = ctx.like
        with torch.cuda.device(dev):
            coeff = grad_output.to(dtype=torch.float64).expand(B, K).contiguous()
            gx, gy = torch.empty(xs, dtype=dtype, device=dev), torch.empty(ys, dtype=dtype, device=dev)
            _lib.check(lib().compute_rnnt_path_edges(_ptr(frames), coeff.data_ptr(), _ptr(boundary), S, T, B, K,
                                                     int(modified), _ptr(gx), gy.data_ptr(),
                                                     _side.options(dev, 0, T, S + 1), _DT[dtype]),
                       "compute_rnnt_path_edges")
        return gx, gy, None, None, None


def path_scores(px, py, frames, boundary=None, validate=True):
    """W(path) (B, K) float64 of the alignments `frames` (B, K, S) int32 -- or (B, S), K = 1 -- in `best_path`'s convention,
    from `sample_paths`, `best_path` or a forced alignment; differentiable in px and py (the gradient is the paths' edge
    indicator times grad_output, summed over k).  A row of frames that is not a path of its rectangle scores NaN and gets
    no gradient."""
    B, S, T, modified = _certified(px, py, boundary, validate, "path_scores")
    frames, K = _certify_frames(frames, py)
    return _PathScores.apply(px, py, frames, boundary, (B, S, T, modified, K))
