"""Best-path (Viterbi) alignment of the Token-and-Duration Transducer over libwarprnnt_tdt_align.so
(include/rnnt_tdt_align.h): per token the frame at which it is emitted and the duration the model chose for it.

    score, frames, durs = tdt_align(logits, labels, act_lens, label_lens, durations=[0, 1, 2, 3, 4], blank=A - 1)
    # frames[b, u]: the frame of label u (the token's timestamp); durs[b, u]: its duration; -1 behind label_lens[b]

The library is loaded on the first call; a missing library is an error (_side.py).
"""
import ctypes as C

import torch

from . import _lib, _side
from .tdt import _certify, durations_array

__all__ = ["tdt_align", "library_path"]

_DT, _P = _side.DT, _side.P
EXPORTS = {
    "get_workspace_size_tdt_align": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "compute_tdt_align": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P,
                                    _lib.rnntOptions, C.c_int]),
}
_LIB = _side.Library("libwarprnnt_tdt_align.so", "the TDT alignment", EXPORTS)
library_path, lib = _LIB.path, _LIB.load


def workspace_bytes(maxT, maxU, minibatch, num_durations, dtype_code):
    return _LIB.workspace_bytes("get_workspace_size_tdt_align", maxT, maxU, minibatch, num_durations, dtype_code)


def tdt_align(acts, labels, act_lens, label_lens, durations, blank=0, sigma=0.0, validate=True):
    """The best path of raw TDT logits (N, T, U, A + D) -> (score, frames, durs).

    The arguments are `rnnt_loss_tdt`'s.  score (N,) float64: the natural-log weight of the best path (-inf: no path, NaN: a
    non-finite row inside the lattice or lengths that do not fit).  frames, durs (N, U - 1) int32: for u < label_lens[b] the
    frame at which label u is emitted and its duration value, -1 behind (and everywhere when the score is not finite).  Runs
    under no_grad; validate=False skips the checks that read the lengths back: the call then only enqueues."""
    dur = durations_array(durations)
    D = len(dur)
    A = _certify(acts, labels, act_lens, label_lens, D, blank, validate, "the TDT alignment")
    B, T, U, _ = acts.shape
    code, dev = _DT[acts.dtype], acts.device
    with torch.no_grad(), torch.cuda.device(dev):
        score = torch.empty(B, dtype=torch.float64, device=dev)
        frames = torch.empty((B, U - 1), dtype=torch.int32, device=dev)
        durs = torch.empty((B, U - 1), dtype=torch.int32, device=dev)
        ws = torch.empty(workspace_bytes(T, U, B, D, code), dtype=torch.uint8, device=dev)
        spare = score.data_ptr()                                        # maxU == 1: never read, never written
        _lib.check(lib().compute_tdt_align(acts.data_ptr(), dur, D, float(sigma), labels.data_ptr() if U > 1 else spare,
                                           label_lens.data_ptr(), act_lens.data_ptr(), A, B, score.data_ptr(),
                                           frames.data_ptr() if U > 1 else spare, durs.data_ptr() if U > 1 else spare,
                                           ws.data_ptr(), _side.options(dev, blank, T, U), code), "compute_tdt_align")
    return score, frames, durs
