"""The joiner's hidden tensor act(f[b, t, :] + g[b, u, :]) of a transducer, written directly in the layout a loss of this package
reads, over libwarprnnt_joiner.so (include/rnnt_joiner.h): padded (N, T, U, H) for `RNNTLoss`, packed (sum_b T_b (L_b + 1), H)
for `RNNTLossPacked`, pruned (N, T, S, H) for `RNNTLossPruned` / `PrunedStreamingRNNTLoss`.  The forward is one write of the
tensor; the backward reads the incoming gradient once and writes df and dg, bit-identical from run to run.

    h = joiner_packed(f, g, act_lens, label_lens, "relu")                 # f (N, T, H) encoder, g (N, maxU, H) predictor
    loss = RNNTLossPacked()(linear(h), labels, act_lens, label_lens)

    h = joiner_pruned(f, g, ranges, S, act_lens)                          # ranges from warprnnt_pytorch.pruned.prune_ranges
    loss = RNNTLossPruned()(linear(h), labels, act_lens, label_lens, ranges)

The recipes are INTEGRATION.md section 18.  The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side
from .packed import row_offsets

__all__ = ["joiner_padded", "joiner_packed", "joiner_pruned", "TransducerJoint", "library_path"]

_DT, _P = _side.DT, _side.P
_TAIL = [C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]
EXPORTS = {
    "get_workspace_size_joiner": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_rnnt_joiner_fwd": (C.c_int, [_P, _P, _P] + _TAIL),
    "compute_rnnt_joiner_bwd": (C.c_int, [_P, _P, _P, _P] + _TAIL),
}
_LIB = _side.Library("libwarprnnt_joiner.so", "the fused joiner", EXPORTS)
library_path, lib = _LIB.path, _LIB.load

PADDED, PACKED, PRUNED = 0, 1, 2
ACTIVATIONS = {"identity": 0, "relu": 1, "tanh": 2}


def workspace_bytes(T, U, S, H, minibatch, layout, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_joiner", T, U, S, H, minibatch, layout, dtype_code)


def act_code(activation):
    if not isinstance(activation, str) or activation not in ACTIVATIONS:
        raise ValueError("activation must be 'identity', 'relu' or 'tanh', got %r" % (activation,))
    return ACTIVATIONS[activation]


def _check_fg(f, g):
    """The checks of f and g that read no device memory."""
    for var, name in ((f, "f"), (g, "g")):
        if not isinstance(var, torch.Tensor) or var.dim() != 3:
            raise ValueError("%s must be a 3D tensor" % name)
    if not f.is_cuda or not g.is_cuda:
        raise ValueError("the fused joiner runs on the GPU only: f is on %s, g is on %s" % (f.device, g.device))
    if f.device != g.device:
        raise ValueError("f and g must be on one device: %s and %s" % (f.device, g.device))
    if f.dtype != g.dtype:
        raise ValueError("f and g must have one dtype: %s and %s" % (f.dtype, g.dtype))
    if f.dtype not in _DT:
        raise ValueError("f and g must be torch.float32, float64, bfloat16 or float16")
    if not f.is_contiguous() or not g.is_contiguous():
        raise ValueError("f and g must be contiguous")
    if f.shape[0] != g.shape[0] or f.shape[2] != g.shape[2] or 0 in f.shape or 0 in g.shape:
        raise ValueError("f must be (N, T, H) and g (N, maxU, H): got %s and %s" % (tuple(f.shape), tuple(g.shape)))


def _check_index(t, name, shape, dtype, dev):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError("%s must be a %s tensor" % (name, dtype))
    if t.device != dev:
        raise ValueError("%s must be on the device of f (%s): it is on %s" % (name, dev, t.device))
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s must be contiguous of shape %s" % (name, tuple(shape)))


def _check(f, g, layout, ranges, S, offsets, label_lens, act_lens, validate):
    _check_fg(f, g)
    N, T, _ = f.shape
    U = g.shape[1]
    _check_index(act_lens, "act_lens", (N,), torch.int32, f.device)
    _check_index(label_lens, "label_lens", (N,), torch.int32, f.device)
    _check_index(offsets, "offsets", (N + 1,), torch.int64, f.device)
    _check_index(ranges, "ranges", (N, T), torch.int32, f.device)
    if layout == PRUNED and not 1 <= S <= U:
        raise ValueError("S must be in [1, maxU] = [1, %d]" % U)
    if validate:                                       # the device-to-host reads
        if act_lens is not None and (int(act_lens.min()) < 0 or int(act_lens.max()) > T):
            raise ValueError("act_lens exceed f: T = %d" % T)
        if label_lens is not None and (int(label_lens.min()) < 0 or int(label_lens.max()) > U - 1):
            raise ValueError("label_lens exceed g: maxU = %d" % U)


class _Joiner(Function):
    """compute_rnnt_joiner_fwd / _bwd.  Returns (out, flags): flags = the per-sample bad-start flags of the pruned layout
    (int32 (N,), not differentiable; None elsewhere)."""

    @staticmethod
    def forward(ctx, f, g, layout, act, ranges, S, offsets, label_lens, act_lens, rows, validate):
        _check(f, g, layout, ranges, S, offsets, label_lens, act_lens, validate)
        N, T, H = f.shape
        U = g.shape[1]
        dev, code = f.device, _DT[f.dtype]
        shape = {PADDED: (N, T, U, H), PACKED: (rows, H), PRUNED: (N, T, S, H)}[layout]
        ptr = lambda t: None if t is None else t.data_ptr()                 # noqa: E731
        with torch.cuda.device(dev):
            out = torch.empty(shape, dtype=f.dtype, device=dev)
            ws = torch.empty(workspace_bytes(T, U, S, H, N, layout, code), dtype=torch.uint8, device=dev)
            tail = (layout, act, ptr(ranges), S, ptr(offsets), ptr(label_lens), ptr(act_lens), T, U, H, N)
            _lib.check(lib().compute_rnnt_joiner_fwd(f.data_ptr(), g.data_ptr(), out.data_ptr(), *tail, ws.data_ptr(),
                                                     _side.options(dev, 0, T, U), code), "compute_rnnt_joiner_fwd")
            flags = None
            if layout == PRUNED:
                at = -ws.data_ptr() % 256
                flags = ws[at:at + 4 * N].view(torch.int32)
                if validate:
                    bad = torch.nonzero(flags).flatten().tolist()
                    if bad:
                        raise ValueError("ranges of sample %d start outside [0, maxU - 1] = [0, %d]" % (bad[0], U - 1))
        ctx.tail, ctx.sizes = tail, (N, T, U, H, code)
        index = [t for t in (ranges, offsets, label_lens, act_lens) if t is not None]
        ctx.save_for_backward(*([out] if act != 0 else []), *index)      # identity: nothing but the index tensors
        ctx.has_out = act != 0
        if flags is None:
            flags = torch.empty(0, dtype=torch.int32, device=dev)
        ctx.mark_non_differentiable(flags)
        return out, flags

    @staticmethod
    def backward(ctx, dout, _dflags):
        N, T, U, H, code = ctx.sizes
        out = ctx.saved_tensors[0] if ctx.has_out else None
        dev = dout.device
        dout = dout.contiguous()
        with torch.cuda.device(dev):
            df = torch.empty((N, T, H), dtype=dout.dtype, device=dev)
            dg = torch.empty((N, U, H), dtype=dout.dtype, device=dev)
            ws = torch.empty(workspace_bytes(T, U, ctx.tail[3], H, N, ctx.tail[0], code), dtype=torch.uint8, device=dev)
            _lib.check(lib().compute_rnnt_joiner_bwd(None if out is None else out.data_ptr(), dout.data_ptr(), df.data_ptr(),
                                                     dg.data_ptr(), *ctx.tail, ws.data_ptr(), _side.options(dev, 0, T, U),
                                                     code), "compute_rnnt_joiner_bwd")
        return (df, dg) + (None,) * 9


def joiner_padded(f, g, act_lens=None, label_lens=None, activation="tanh", validate=True):
    """(N, T, maxU, H): row (b, t, u) = act(f[b, t] + g[b, u]) for t < act_lens[b] and u <= label_lens[b], exact zeros
    elsewhere (lengths None: every row is real) -- the input of `RNNTLoss` behind the joiner's Linear.  f (N, T, H) and
    g (N, maxU, H) contiguous, of one dtype, on one GPU; lengths int32 (N,) there.  validate=False skips the checks that read
    device memory: the call then only enqueues."""
    return _Joiner.apply(f, g, PADDED, act_code(activation), None, 0, None, label_lens, act_lens, None, validate)[0]


def joiner_packed(f, g, act_lens, label_lens, activation="tanh", offsets=None, rows=None, validate=True):
    """(R, H) with row offsets[b] + t (label_lens[b] + 1) + u = act(f[b, t] + g[b, u]): the layout of `RNNTLossPacked`, no padding
    anywhere.  offsets = packed.row_offsets(act_lens, label_lens) when None; rows = R = offsets[-1], read back from the device
    when None -- the one device-to-host read.  Given `rows` and validate=False the call only enqueues (and can be captured in a
    graph)."""
    act = act_code(activation)
    if act_lens is None or label_lens is None:
        raise ValueError("the packed layout needs act_lens and label_lens")
    if offsets is None:
        _check_fg(f, g)
        offsets = row_offsets(act_lens, label_lens)
    if rows is None:
        rows = int(offsets[-1])
    elif validate and int(offsets[-1]) != int(rows):
        raise ValueError("rows = %d, offsets[-1] = %d" % (int(rows), int(offsets[-1])))
    return _Joiner.apply(f, g, PACKED, act, None, 0, offsets, label_lens, act_lens, int(rows), validate)[0]


def joiner_pruned(f, g, ranges, S, act_lens=None, activation="tanh", validate=True, return_flags=False):
    """(N, T, S, H): row (b, t, k) = act(f[b, t] + g[b, min(ranges[b, t] + k, maxU - 1)]) -- act(am_p + lm_p) of
    `pruned.prune_inputs` in one write, and in the backward no scatter.  ranges int32 (N, T) window starts (`prune_ranges`);
    with act_lens, frames t >= act_lens[b] are zeros and their ranges are not read.  A start outside [0, maxU - 1] raises
    ValueError under validate=True; with validate=False that sample's rows are zeros, it gets no gradient, and its flag is 1
    in the int32 (N,) tensor `return_flags=True` returns behind the output."""
    out, flags = _Joiner.apply(f, g, PRUNED, act_code(activation), ranges, int(S), None, None, act_lens, None, validate)
    return (out, flags) if return_flags else out


class TransducerJoint(Module):
    """forward(f, g, f_len, g_len) in the shape of apex.contrib.transducer.TransducerJoint's call: f (N, T, H), g (N, maxU, H),
    f_len the frames and g_len the rows of g that are real per sample (g_len = label_lens + 1), int32 or int64 on the device.
    pack_output=False: the padded (N, T, maxU, H) tensor, zeros in the padding; pack_output=True: the packed (R, H) tensor.
    activation "identity" | "relu" | "tanh" (apex's relu=True is "relu", its default "identity").  Out of scope: dropout, apex's
    `batch_offset` / `packed_batch` arguments (the offsets are computed here) and its masks."""

    def __init__(self, activation="relu", pack_output=False, validate=True):
        super().__init__()
        act_code(activation)
        self.activation, self.pack_output, self.validate = activation, bool(pack_output), validate

    def forward(self, f, g, f_len, g_len):
        act_lens = f_len.to(torch.int32)
        label_lens = (g_len - 1).to(torch.int32)
        if self.pack_output:
            return joiner_packed(f, g, act_lens, label_lens, self.activation, validate=self.validate)
        return joiner_padded(f, g, act_lens, label_lens, self.activation, self.validate)
