"""What the side modules (the losses pruned, tdt, hat, mblank, and tdt_align) share: the loader of a side library, its
workspace-size cache, the checks of (logits, labels, act_lens, label_lens) and, for the losses, the skeleton of the two-phase
autograd function.

Each side library is a separate shared object next to libwarprnnt.so, loaded on the first call (`import warprnnt_pytorch` does
not need it); a missing library is an error, there is no fallback.  The ctypes table (`EXPORTS`), the checks of its own
arguments and the literal calls of the C entries stay in the loss's module.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._checks import check_contiguous, check_dim, check_type, check_gpu_arguments

DT = {torch.float32: _lib.DT_F32, torch.float64: _lib.DT_F64, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}
P = C.c_void_p


class Library:
    """One side library: its handle, and the workspace sizes it has been asked for.  The cache is the library's own: the same
    (maxT, maxU, N, dtype) is a different size in each."""

    def __init__(self, filename, loss, exports):
        self.filename, self.loss, self.exports = filename, loss, exports
        self._handle = None
        self._sizes = {}

    def path(self):
        """Next to libwarprnnt.so: WARP_RNNT_PATH (a directory, or the main library's file), the installed package, the source
        tree."""
        return os.path.join(os.path.dirname(_lib.library_path()), self.filename)

    def load(self):
        if self._handle is None:
            path = self.path()
            if not os.path.exists(path):
                raise ImportError("%s not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for %s." % (self.filename, path, self.loss))
            h = C.CDLL(path)
            for name, (res, args) in self.exports.items():
                fn = getattr(h, name)   # AttributeError if the symbol is missing: intended
                fn.restype, fn.argtypes = res, args
            self._handle = h
        return self._handle

    def workspace_bytes(self, entry, *sizes):
        """`entry`(*sizes, size_t*) of this library (a get_workspace_size_*: host arithmetic), asked once per `sizes`."""
        n = self._sizes.get(sizes)
        if n is None:
            c = C.c_size_t(0)
            _lib.check(getattr(self.load(), entry)(*(int(v) for v in sizes), C.byref(c)), entry)
            n = self._sizes[sizes] = c.value
        return n


def options(dev, blank, T, U):
    return _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream,
                            blank_label=int(blank), maxT=int(T), maxU=int(U), batch_first=True)


def check_reduction(reduction):
    if reduction not in ("none", "sum", "mean"):
        raise ValueError("reduction must be 'none', 'sum' or 'mean'")


def certify(logits, labels, act_lens, label_lens, validate, gpu_only):
    """The checks every side loss makes of its four tensors.  `gpu_only`: the loss's message for logits that are not on a GPU
    (it may name them as %(device)s).  validate: read the lengths back for T == max(act_lens), labels.shape[1] ==
    max(label_lens) -- the one device-to-host read."""
    check_type(labels, torch.int32, "labels")
    check_type(label_lens, torch.int32, "label_lengths")
    check_type(act_lens, torch.int32, "lengths")
    for var, name in ((logits, "logits"), (labels, "labels"), (act_lens, "lengths"), (label_lens, "label_lengths")):
        check_contiguous(var, name)
    check_dim(logits, 4, "logits")
    check_dim(labels, 2, "labels")
    check_dim(act_lens, 1, "lengths")
    check_dim(label_lens, 1, "label_lengths")
    if not logits.is_cuda:
        raise ValueError(gpu_only % {"device": logits.device})
    if logits.dtype not in DT:
        raise TypeError("logits must be torch.float32, float64, bfloat16 or float16")
    B = logits.shape[0]
    if act_lens.shape[0] != B or label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a length per example.")
    check_gpu_arguments(logits, labels, act_lens, label_lens)
    if validate:
        max_t, max_l = torch.stack((act_lens, label_lens)).amax(1).tolist()
        if logits.shape[1] != max_t:
            raise ValueError("Input length mismatch")
        if labels.shape[1] != max_l:
            raise ValueError("Output length mismatch")


def _cost_dtype(logits):
    return torch.float64 if logits.dtype == torch.float64 else torch.float32


def forward(ctx, logits, labels, workspace_size, reduction, call, what, also_save=()):
    """The forward half of a two-phase loss.  call(costs, labels, workspace, prepare_backward) -> status makes the loss's
    *_fwd call (named `what`) on these device pointers.  Leaves the logits, the workspace and mean_scale in ctx; `also_save`:
    further tensors the backward half needs (ctx.saved_tensors holds them behind the logits)."""
    B, dev = logits.shape[0], logits.device
    need_grad = logits.requires_grad
    with torch.cuda.device(dev):
        costs = torch.empty(B, dtype=_cost_dtype(logits), device=dev)
        ws = torch.empty(workspace_size, dtype=torch.uint8, device=dev)
        lab_ptr = labels.data_ptr() if labels.numel() else costs.data_ptr()    # maxU == 1: never read
        _lib.check(call(costs.data_ptr(), lab_ptr, ws.data_ptr(), 1 if need_grad else 0), what)
    ctx.save_for_backward(logits, *also_save)
    ctx.workspace = ws if need_grad else None
    ctx.mean_scale = 1.0 / B if reduction == "mean" else 1.0
    if reduction == "sum":
        return costs.sum(0, keepdim=True)
    if reduction == "mean":
        return costs.mean(0, keepdim=True)
    return costs


def backward(ctx, logits, grad_output, call, what):
    """The backward half: call(gradients, grad_scale, workspace) -> status makes the loss's *_bwd call (named `what`), which
    streams the gradient once with grad_output and the 1/N of 'mean' folded into its per-sample scale."""
    B, dev = logits.shape[0], logits.device
    with torch.cuda.device(dev):
        scale = (grad_output.reshape(-1).to(device=dev, dtype=_cost_dtype(logits)).expand(B) * ctx.mean_scale).contiguous()
        grads = torch.empty_like(logits)
        _lib.check(call(grads.data_ptr(), scale.data_ptr(), ctx.workspace.data_ptr()), what)
        ctx.workspace.record_stream(torch.cuda.current_stream(dev))
    return grads
