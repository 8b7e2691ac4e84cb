"""Token-and-Duration Transducer (TDT) loss (Xu et al., ICML 2023) over libwarprnnt_tdt.so (include/rnnt_tdt.h).

The recipe:

    logits = joiner(enc, pred)                       # (N, T, U, A + D): A token logits (blank included), D duration logits
    loss = TDTLoss(durations=[0, 1, 2, 3, 4], blank=A - 1, sigma=0.05)(logits, labels, act_lens, label_lens)

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

from torch.autograd import Function
from torch.nn import Module

from . import _lib, _side

__all__ = ["rnnt_loss_tdt", "TDTLoss", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_tdt": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_tdt_loss": (C.c_int, [_P, _P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P,
                                   _lib.rnntOptions, C.c_int]),
    "compute_tdt_loss_fwd": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P, _lib.rnntOptions,
                                       C.c_int, C.c_int]),
    "compute_tdt_loss_bwd": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_tdt.so", "the TDT loss", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, num_durations, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_tdt", maxT, maxU, minibatch, num_durations, dtype_code)


def durations_array(durations):
    """The host int array of the C-ABI, checked as include/rnnt_tdt.h asks."""
    d = [int(v) for v in durations]
    if not 1 <= len(d) <= 8:
        raise ValueError("1 to 8 durations, got %d" % len(d))
    if d[0] < 0 or any(b <= a for a, b in zip(d, d[1:])) or not 1 <= d[-1] <= 64:
        raise ValueError("durations must be strictly increasing, non-negative, the largest in [1, 64]: %s" % (d,))
    return (C.c_int * len(d))(*d)


def _certify(logits, labels, act_lens, label_lens, D, blank, validate, what="the TDT loss"):
    """The checks of TDT logits (N, T, U, A + D) -> A; `what` names the entry in the GPU-only refusal (tdt_align.py's too)."""
    _side.certify(logits, labels, act_lens, label_lens, validate,
                  what + " runs on the GPU only: logits are on %(device)s")
    if logits.shape[2] != labels.shape[1] + 1:
        raise ValueError("logits.shape[2] must be labels.shape[1] + 1")
    A = logits.shape[3] - D
    if A < 1:
        raise ValueError("logits.shape[3] = %d leaves no token column next to %d durations" % (logits.shape[3], D))
    if not 0 <= int(blank) < A:
        raise ValueError("blank = %d is not a token column (A = %d)" % (int(blank), A))
    return A


class _TDT(Function):
    """Two-phase (compute_tdt_loss_fwd / _bwd, under _side.forward / _side.backward)."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, durations, blank, sigma, reduction, validate):
        dur = durations_array(durations)
        D = len(dur)
        A = _certify(logits, labels, act_lens, label_lens, D, blank, validate)
        B, T, U, _ = logits.shape
        code = _DT[logits.dtype]

        def call(costs, lab_ptr, ws, prepare_backward):
            return lib().compute_tdt_loss_fwd(logits.data_ptr(), dur, D, float(sigma), lab_ptr, label_lens.data_ptr(),
                                              act_lens.data_ptr(), A, B, costs, ws,
                                              _side.options(logits.device, blank, T, U), code, prepare_backward)
        ctx.dur, ctx.A, ctx.blank = dur, A, int(blank)
        return _side.forward(ctx, logits, labels, workspace_bytes(T, U, B, D, code), reduction, call, "compute_tdt_loss_fwd")

    @staticmethod
    def backward(ctx, grad_output):
        (logits,) = ctx.saved_tensors
        B, T, U, _ = logits.shape

        def call(grads, scale, ws):
            return lib().compute_tdt_loss_bwd(logits.data_ptr(), grads, scale, ctx.dur, len(ctx.dur), ctx.A, B, ws,
                                              _side.options(logits.device, ctx.blank, T, U), _DT[logits.dtype])
        grads = _side.backward(ctx, logits, grad_output, call, "compute_tdt_loss_bwd")
        return grads, None, None, None, None, None, None, None, None


def rnnt_loss_tdt(acts, labels, act_lens, label_lens, durations, blank=0, sigma=0.0, reduction="mean", validate=True):
    """TDT loss of raw logits (N, T, U, A + D): the first A columns are tokens (blank = `blank`), the last D the logits of
    `durations` (1 to 8 ints, strictly increasing, non-negative, the largest in [1, 64]).  sigma: the logit
    under-normalisation of the token log-probs (natural log).  labels (N, U - 1), act_lens, label_lens (N,) int32 on the
    device of the logits.  Costs float32 (float64 for float64 logits); reduction 'none' | 'sum' | 'mean' as `rnnt_loss`.
    validate=False skips the checks that read the lengths back: the call then only enqueues."""
    _side.check_reduction(reduction)
    return _TDT.apply(acts, labels, act_lens, label_lens, tuple(int(d) for d in durations), blank, float(sigma), reduction,
                      validate)


class TDTLoss(Module):
    """Module form of `rnnt_loss_tdt`: forward(acts, labels, act_lens, label_lens)."""

    def __init__(self, durations, blank=0, sigma=0.0, reduction="mean"):
        super().__init__()
        durations_array(durations)
        self.durations = tuple(int(d) for d in durations)
        self.blank, self.sigma, self.reduction = blank, float(sigma), reduction

    def forward(self, acts, labels, act_lens, label_lens):
        return rnnt_loss_tdt(acts, labels, act_lens, label_lens, self.durations, self.blank, self.sigma, self.reduction)
