"""Transducer lattice distillation loss (Panchapagesan et al., ICASSP 2021) over libwarprnnt_kd.so (include/rnnt_kd.h).

At every lattice node (t, u) the KL divergence from the teacher's output distribution to the student's, by default
collapsed to the three classes {blank, the correct label y_u, everything else}.  The recipe:

    with torch.no_grad():
        teacher_logits = teacher_joiner(t_enc, t_pred)           # (N, T, U, A), the student's shape and dtype
    logits = joiner(enc, pred)
    loss = RNNTLoss()(logits, labels, act_lens, label_lens) \\
        + lam * tau ** 2 * TransducerKDLoss(temperature=tau)(logits, teacher_logits, labels, act_lens, label_lens)

The kernels read the teacher once and the student twice and write the gradient once; no tensor of the logits' size is
kept.  `kd_loss_torch` is the same loss in plain torch -- the route this module replaces.

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C
import math

import torch
from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side

__all__ = ["rnnt_kd_loss", "TransducerKDLoss", "kd_loss_torch", "library_path"]

_DT, _P = _side.DT, _side.P
MODES = {"collapsed": 0, "full": 1}
EXPORTS = {
    "get_workspace_size_kd": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_kd_loss": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int, C.c_int,
                                  C.c_float]),
    "compute_kd_loss_fwd": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions, C.c_int, C.c_int,
                                      C.c_float, C.c_int]),
    "compute_kd_loss_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int, C.c_int, C.c_float]),
}
_LIB = _side.Library("libwarprnnt_kd.so", "the distillation loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_kd", maxT, maxU, minibatch, dtype_code)


def _check_own(logits, teacher, blank, mode, temperature):
    """The checks of this loss's own arguments (none of them needs a device)."""
    if mode not in MODES:
        raise ValueError("mode must be 'collapsed' or 'full', got %r" % (mode,))
    tau = float(temperature)
    if not (math.isfinite(tau) and tau > 0.0):
        raise ValueError("temperature must be finite and positive, got %r" % (temperature,))
    if teacher.shape != logits.shape:
        raise ValueError("teacher logits %s must have the shape of the student's %s" % (tuple(teacher.shape), tuple(logits.shape)))
    if teacher.dtype != logits.dtype:
        raise TypeError("teacher logits must be %s as the student's, got %s" % (logits.dtype, teacher.dtype))
    if teacher.device != logits.device:
        raise ValueError("teacher logits must be on the device of the student's (%s), got %s" % (logits.device, teacher.device))
    if not teacher.is_contiguous():
        raise ValueError("teacher logits must be contiguous")
    if logits.dim() == 4:
        A = logits.shape[3]
        if A < 2:
            raise ValueError("the distillation loss needs a column besides the blank: logits.shape[3] = %d" % A)
        if not 0 <= int(blank) < A:
            raise ValueError("blank = %d is not a column (A = %d)" % (int(blank), A))


def _certify(logits, teacher, labels, act_lens, label_lens, blank, mode, temperature, validate):
    _check_own(logits, teacher, blank, mode, temperature)
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  "the distillation loss runs on the GPU only: logits are on %(device)s")
    if logits.shape[2] != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")


class _KD(Function):
    """Two-phase (compute_kd_loss_fwd / _bwd, under _side.forward / _side.backward).  Full mode's gradient stream reads the
    teacher, which then travels to backward with the logits; collapsed mode's does not, and the teacher is not kept.  The
    teacher gets no gradient."""

    @staticmethod
    def forward(ctx, logits, teacher, labels, act_lens, label_lens, blank, mode, temperature, reduction, validate):
        _certify(logits, teacher, labels, act_lens, label_lens, blank, mode, temperature, validate)
        B, T, U, A = logits.shape
        code = _DT[logits.dtype]
        teacher = teacher.detach()
        ctx.blank, ctx.mode, ctx.tau = int(blank), MODES[mode], float(temperature)

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_kd_loss_fwd(logits.data_ptr(), teacher.data_ptr(), lab_ptr, label_lens.data_ptr(),
                                             act_lens.data_ptr(), A, B, costs, ws,
                                             _side.options(logits.device, blank, T, U), code, ctx.mode, ctx.tau,
                                             prepare_backward)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, code), reduction, call, "compute_kd_loss_fwd",
                             also_save=(teacher,) if ctx.mode == 1 else ())

    @staticmethod
    def backward(ctx, grad_output):
        logits, teacher = (tuple(ctx.saved_tensors) + (None,))[:2]
        teacher_ptr = teacher.data_ptr() if teacher is not None else None
        B, T, U, A = logits.shape

        def call(grads, scale, ws):
            return lib().compute_kd_loss_bwd(logits.data_ptr(), teacher_ptr, grads, scale, A, B, ws,
                                             _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype], ctx.mode,
                                             ctx.tau)
        grads = _side.backward(ctx, logits, grad_output, call, "compute_kd_loss_bwd")
        return grads, None, None, None, None, None, None, None, None, None


def rnnt_kd_loss(acts, teacher_acts, labels, act_lens, label_lens, blank=0, mode="collapsed", temperature=1.0,
                 reduction="mean", validate=True):
    """Distillation loss of the student's raw logits `acts` against the teacher's `teacher_acts`, both (N, T, U, A) of one
    dtype on one GPU, contiguous.  labels (N, U - 1), act_lens, label_lens (N,) int32 on that device.  Per sample the sum over
    its lattice rows (t < T_b, u <= L_b) of KL(q || p), p = softmax(acts / temperature), q = softmax(teacher_acts /
    temperature): mode 'collapsed' over the classes {blank, y_u, rest}, 'full' over every column.  No temperature^2 factor
    and no division by the number of rows: the caller scales.  Costs float32 (float64 for float64 logits); reduction 'none' |
    'sum' | 'mean' as `rnnt_loss`.  Only `acts` gets a gradient (a teacher that requires grad gets None).  validate=False
    skips the checks that read the lengths back: the call then only enqueues."""
    _side.check_reduction(reduction)
    return _KD.apply(acts, teacher_acts, labels, act_lens, label_lens, blank, mode, temperature, reduction, validate)


class TransducerKDLoss(Module):
    """Module form of `rnnt_kd_loss`: forward(acts, teacher_acts, labels, act_lens, label_lens)."""

    def __init__(self, blank=0, mode="collapsed", temperature=1.0, reduction="mean"):
        super().__init__()
        _side.check_reduction(reduction)
        if mode not in MODES:
            raise ValueError("mode must be 'collapsed' or 'full', got %r" % (mode,))
        self.blank, self.mode, self.temperature, self.reduction = int(blank), mode, float(temperature), reduction

    def forward(self, acts, teacher_acts, labels, act_lens, label_lens):
        return rnnt_kd_loss(acts, teacher_acts, labels, act_lens, label_lens, self.blank, self.mode, self.temperature,
                            self.reduction)


def kd_loss_torch(acts, teacher_acts, labels, act_lens, label_lens, blank=0, mode="collapsed", temperature=1.0,
                  reduction="mean"):
    """The same loss in plain differentiable torch, on any device: log_softmax of both tensors, the classes gathered, the
    padding masked.  It holds several tensors of the logits' size -- the route the kernels replace, and what tools/kd_bench.py
    compares them with.  Padding rows may hold anything; the teacher gets no gradient."""
    _side.check_reduction(reduction)
    _check_own(acts, teacher_acts, blank, mode, temperature)
    N, T, U, A = acts.shape
    dev = acts.device
    inside = (torch.arange(T, device=dev)[None, :, None] < act_lens.to(dev)[:, None, None]) & \
             (torch.arange(U, device=dev)[None, None, :] <= label_lens.to(dev)[:, None, None])
    keep = inside[..., None]
    lp = torch.log_softmax(torch.where(keep, acts, torch.zeros_like(acts)) / temperature, -1)
    lq = torch.log_softmax(torch.where(keep, teacher_acts.detach(), torch.zeros_like(acts)) / temperature, -1)
    if MODES[mode] == 0:
        lab = torch.full((N, U), int(blank), dtype=torch.long, device=dev)
        if U > 1:
            has = torch.arange(U - 1, device=dev)[None, :] < label_lens.to(dev)[:, None]
            lab[:, :U - 1] = torch.where(has, labels.to(dev).long().clamp(0, A - 1), lab[:, :U - 1])
        lab = lab[:, None, :, None].expand(N, T, U, 1)
        cols = torch.arange(A, device=dev)
        is_blank = (cols == int(blank)).expand(N, T, U, A)
        is_label = (cols == lab) & ~is_blank
        neg = float("-inf")

        def classes(l):
            return torch.stack((l[..., int(blank)],
                                torch.logsumexp(l.masked_fill(~is_label, neg), -1),
                                torch.logsumexp(l.masked_fill(is_blank | is_label, neg), -1)), -1)
        lp, lq = classes(lp), classes(lq)
    q = lq.exp()
    diff = torch.where(q > 0, lq - lp, torch.zeros_like(lp))              # (a class with Q = 0 contributes 0)
    rows = (q * diff).sum(-1)
    costs = torch.where(inside, rows, torch.zeros_like(rows)).sum((1, 2))
    if reduction == "sum":
        return costs.sum(0, keepdim=True)
    if reduction == "mean":
        return costs.mean(0, keepdim=True)
    return costs
