"""The edge log-probabilities of a transducer lattice from logits: k2 / fast_rnnt's `get_rnnt_logprobs_joint` and
`get_rnnt_logprobs_pruned`, over libwarprnnt_logprobs.so (include/rnnt_logprobs.h).  One read of the logits gives px, py and the
normaliser lse; the backward reads the logits once more and writes their gradient once -- no log-softmax tensor, no gathers, no
permutes and no cat are kept for autograd.  The edges can be edited before the lattice:

    px, py, lse = get_rnnt_logprobs_joint(logits, symbols, blank, boundary, return_lse=True)
    py = py - ilm_scale * ilm_py                                                  # the caller's own edge weights
    scores = mutual_information_recursion(px, py, boundary)                       # warprnnt_pytorch.mi
    loss = -scores.sum() + 1e-4 * (lse ** 2).sum()                                # a z-loss on the normaliser

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib, _side

__all__ = ["get_rnnt_logprobs_joint", "get_rnnt_logprobs_pruned", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "compute_rnnt_logprobs_fwd": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P,
                                            _lib.rnntOptions, C.c_int]),
    "compute_rnnt_logprobs_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                            _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_logprobs.so", "the fused edge log-probabilities", EXPORTS)
library_path, lib = _LIB.path, _LIB.load

RNNT_TYPES = {"regular": 0, "modified": 1}


def type_code(rnnt_type):
    if not isinstance(rnnt_type, str) or rnnt_type not in RNNT_TYPES:
        raise ValueError("rnnt_type must be 'regular' or 'modified', got %r" % (rnnt_type,))
    return RNNT_TYPES[rnnt_type]


def _certify(logits, symbols, ranges, blank, boundary, validate):
    """-> (B, T, U, C, K, symbols int32, starts int32 or None).  Everything but the values of boundary, symbols and ranges is
    checked from the tensors' descriptions; validate: the one device-to-host read."""
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise ValueError("logits must be a 4D tensor")
    if not torch.is_tensor(symbols) or symbols.dim() != 2 or symbols.dtype not in (torch.int32, torch.int64):
        raise ValueError("symbols must be a 2D int32 or int64 tensor")
    if logits.dtype not in _DT:
        raise ValueError("logits must be torch.float32, float64, bfloat16 or float16")
    if not logits.is_cuda:
        raise ValueError("the fused edge log-probabilities run on the GPU only: logits are on %s" % logits.device)
    B, T, Kp, Cn = logits.shape
    S = symbols.shape[1]
    U = S + 1
    if 0 in logits.shape or symbols.shape[0] != B:
        raise ValueError("logits must be (B, T, S + 1 or K, C) and symbols (B, S): got %s and %s"
                         % (tuple(logits.shape), tuple(symbols.shape)))
    if not logits.is_contiguous():
        raise ValueError("logits must be contiguous")
    if not 0 <= int(blank) < Cn:
        raise ValueError("termination_symbol must be in [0, C) = [0, %d)" % Cn)
    starts = None
    if ranges is None:
        K = 0
        if Kp != U:
            raise ValueError("joint logits must be (B, T, S + 1, C): got %s for S = %d" % (tuple(logits.shape), S))
    else:
        K = Kp
        if not torch.is_tensor(ranges) or ranges.dtype not in (torch.int32, torch.int64) or ranges.dim() not in (2, 3):
            raise ValueError("ranges must be an integer tensor: (B, T) starts, or k2's (B, T, K) indices")
        if tuple(ranges.shape[:2]) != (B, T) or (ranges.dim() == 3 and ranges.shape[2] != K):
            raise ValueError("ranges must be (B, T) or (B, T, K) for logits %s: got %s" % (tuple(logits.shape), tuple(ranges.shape)))
        if not 1 <= K <= U:
            raise ValueError("pruned logits must be (B, T, K, C) with 1 <= K <= S + 1 = %d" % U)
        starts = (ranges[:, :, 0] if ranges.dim() == 3 else ranges).to(torch.int32).contiguous()
    if boundary is not None:
        if not torch.is_tensor(boundary) or boundary.dtype != torch.int64 or tuple(boundary.shape) != (B, 4):
            raise ValueError("boundary must be an int64 tensor of shape (B, 4)")
        if not boundary.is_contiguous():
            raise ValueError("boundary must be contiguous")
    for t, name in ((symbols, "symbols"), (ranges, "ranges"), (boundary, "boundary")):
        if t is not None and t.device != logits.device:
            raise ValueError("%s must be on the device of logits (%s): it is on %s" % (name, logits.device, t.device))
    sym = symbols.to(torch.int32).contiguous()
    if validate:                                           # the one device-to-host read
        no = torch.zeros((), dtype=torch.bool, device=logits.device)
        bad_sym = ((sym < 0) | (sym >= Cn)).any()
        bad_start = ((starts < 0) | (starts > U - K)).any() if starts is not None else no
        bad_bound = no
        if boundary is not None:
            s0, t0, s1, t1 = boundary.unbind(1)
            bad_bound = ((s0 != 0) | (t0 != 0) | (s1 < 0) | (s1 > S) | (t1 < 0) | (t1 > T)).any()
        flags = torch.stack((bad_sym, bad_start, bad_bound)).tolist()
        if flags[0]:
            raise ValueError("symbols must be in [0, C) = [0, %d)" % Cn)
        if flags[1]:
            raise ValueError("ranges must start in [0, S + 1 - K] = [0, %d]" % (U - K))
        if flags[2]:
            raise ValueError("boundary rows must be [0, 0, s1, t1] with 0 <= s1 <= %d and 0 <= t1 <= %d" % (S, T))
    return B, T, U, Cn, K, sym, starts


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class _Logprobs(Function):
    """compute_rnnt_logprobs_fwd / _bwd.  Saves the logits and lse; the index tensors ride along."""

    @staticmethod
    def forward(ctx, logits, symbols, ranges, blank, boundary, mod, validate):
        B, T, U, Cn, K, sym, starts = _certify(logits, symbols, ranges, blank, boundary, validate)
        code, dev = _DT[logits.dtype], logits.device
        lat = torch.float64 if logits.dtype == torch.float64 else torch.float32
        with torch.cuda.device(dev):
            px = torch.empty((B, U - 1, T + 1 - mod), dtype=lat, device=dev)
            py = torch.empty((B, U, T), dtype=lat, device=dev)
            lse = torch.empty(logits.shape[:3], dtype=lat, device=dev)
            _lib.check(lib().compute_rnnt_logprobs_fwd(logits.data_ptr(), _ptr(sym), _ptr(starts), K, _ptr(boundary), mod, T, U, Cn,
                                                       B, _ptr(px), py.data_ptr(), lse.data_ptr(),
                                                       _side.options(dev, blank, T, U), code), "compute_rnnt_logprobs_fwd")
        ctx.sizes = (B, T, U, Cn, K, mod, int(blank), code)
        ctx.index = (sym, starts, boundary)
        ctx.save_for_backward(logits, lse)
        return px, py, lse

    @staticmethod
    def backward(ctx, px_grad, py_grad, lse_grad):
        B, T, U, Cn, K, mod, blank, code = ctx.sizes
        sym, starts, boundary = ctx.index
        logits, lse = ctx.saved_tensors
        dev = logits.device
        with torch.cuda.device(dev):
            gx = px_grad.contiguous() if px_grad is not None else torch.zeros((B, U - 1, T + 1 - mod), dtype=lse.dtype, device=dev)
            gy = py_grad.contiguous() if py_grad is not None else torch.zeros((B, U, T), dtype=lse.dtype, device=dev)
            gl = lse_grad.contiguous() if lse_grad is not None else None
            dlogits = torch.empty_like(logits)
            _lib.check(lib().compute_rnnt_logprobs_bwd(logits.data_ptr(), lse.data_ptr(), _ptr(sym), _ptr(starts), K, _ptr(boundary),
                                                       mod, _ptr(gx), gy.data_ptr(), _ptr(gl), T, U, Cn, B, dlogits.data_ptr(),
                                                       _side.options(dev, blank, T, U), code), "compute_rnnt_logprobs_bwd")
        return dlogits, None, None, None, None, None, None


def _call(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, return_lse, validate):
    mod = type_code(rnnt_type)
    px, py, lse = _Logprobs.apply(logits, symbols, ranges, int(termination_symbol), boundary, mod, validate)
    return (px, py, lse) if return_lse else (px, py)


def get_rnnt_logprobs_joint(logits, symbols, termination_symbol, boundary=None, rnnt_type="regular", return_lse=False,
                            validate=True):
    """k2's `get_rnnt_logprobs_joint`.  logits (B, T, S + 1, C) of one floating dtype, contiguous, on one GPU; symbols (B, S)
    int32 or int64; boundary None or int64 (B, 4) rows [0, 0, S_b, T_b].  Returns (px, py): px (B, S, T + 1) -- "regular" -- or
    (B, S, T) -- "modified" --, py (B, S + 1, T), float32 (float64 for float64 logits), -inf outside each sample's rectangle;
    with return_lse=True also lse (B, T, S + 1), the rows' logsumexp (exact 0 outside).  Differentiable in logits through all
    three.  validate=False skips the one check that reads device memory: the call then only enqueues."""
    return _call(logits, symbols, None, termination_symbol, boundary, rnnt_type, return_lse, validate)


def get_rnnt_logprobs_pruned(logits, symbols, ranges, termination_symbol, boundary=None, rnnt_type="regular", return_lse=False,
                             validate=True):
    """k2's `get_rnnt_logprobs_pruned`.  logits (B, T, K, C): row (b, t, k) is lattice row ranges[b, t] + k; ranges int32 (B, T)
    frame starts (`pruned.prune_ranges`) or k2's (B, T, K) index tensor, of which [:, :, 0] is used.  Everything else as
    `get_rnnt_logprobs_joint`; lse is (B, T, K).  Positions no window covers are -inf."""
    if ranges is None:
        raise ValueError("the pruned form needs ranges")
    return _call(logits, symbols, ranges, termination_symbol, boundary, rnnt_type, return_lse, validate)
