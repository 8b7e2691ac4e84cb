"""What the -m gpu test modules share (not collected, not a conftest): the kernels a call launched, by name, through
torch.profiler; the dtype tables; device placement at a byte offset; ragged lengths; the C-ABI options; the call forms of a side
library; and, from tests/side_check.py, the cost-and-gradient checker and the per-stage kernel comparison."""
import re
import subprocess

import numpy as np
import torch

from tests.side_check import COST_TOL, assert_stages, check, in_lattice_mask, stages_seen     # noqa: F401  (re-exported)

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "f64": 1, "bf16": 2, "f16": 3}
NAME = {v: k for k, v in TORCH.items()}
CALL = {"f32": "compute_rnnt_loss", "f64": "compute_rnnt_loss_fp64", "bf16": "compute_rnnt_loss_bf16", "f16": "compute_rnnt_loss_fp16"}


# ----------------------------------------------------------------------------- the kernels a call launched
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def demangle(names):
    mangled = [n for n in names if n.startswith("_Z")]
    out = {n: n for n in names}
    if mangled:
        dem = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
        out.update(dict(zip(mangled, dem)))
    return out


def normalise(name):
    """'void rnnt::grad_flat_kernel<rnnt::F32, 1, 2, 1>(float const*, ...)' -> 'rnnt::grad_flat_kernel<rnnt::F32, 1, 2, 1>'"""
    name = re.sub(r"^void ", "", name.strip())
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i].strip()
    return name


def kernels(prof):
    """[normalised kernel name] of the device events a profiler recorded, in order."""
    from torch.autograd import DeviceType
    raw = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    dem = demangle(set(raw))
    return [normalise(dem[n]) for n in raw]


def profiled(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, kernels(prof)


def assert_every_row_reached(forms, cus, also_unreachable=()):
    """Every kernel of a side library's code objects (the table of `forms` at its default of 256 compute units: the library's
    CPU test checks it against the objects) is reached by some case on a device of `cus` compute units, or is listed as
    unreachable."""
    rows = forms.predicted_rows(cus)
    for obj, ks in forms.expected_inventory().items():
        for k in ks:
            assert (obj, k) in rows or (obj, k) in forms.UNREACHABLE or (obj, k) in also_unreachable, (obj, k)


# ----------------------------------------------------------------------------- inputs
def options(T, U, blank=0, stream=None):
    from warprnnt_pytorch import _lib
    s = stream if stream is not None else torch.cuda.current_stream()
    return _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=s.cuda_stream, blank_label=blank, maxT=T, maxU=U,
                            batch_first=True)


def dev(*arrays):
    return [torch.tensor(np.ascontiguousarray(a), device=DEV) for a in arrays]


def place(values, off, dtype):
    """A device tensor of `values` `off` bytes past a 16-byte boundary inside a larger NaN buffer."""
    esz = torch.finfo(dtype).bits // 8
    assert off % esz == 0
    n = values.numel()
    buf = torch.full((n + 32 // esz,), float("nan"), dtype=dtype, device=DEV)
    base = (-buf.data_ptr() % 16) // esz                             # (torch allocations are 256-byte aligned: 0)
    v = buf[base + off // esz: base + off // esz + n].view(values.shape)
    v.copy_(values)
    assert v.data_ptr() % 16 == off
    return v


def ragged_lengths(N, T, U, rng, pair_without_labels=False):
    """Frame and label counts: sample 0 full (maxT / maxU are used), sample 1 with T_b = 1, sample 2 with L_b = 0.
    pair_without_labels (the joint tests' rule): at N = 2, sample 1 gets L_b = 0 as well."""
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    if N > 1:
        tl[1] = 1
    if N > 2:
        ll[2] = 0
    elif N == 2 and pair_without_labels:
        ll[1] = 0
    return tl, ll


# ----------------------------------------------------------------------------- the call forms of a side library
def call_forms(x, form, one, fwd, bwd, ws_bytes, scale=None, grads=None, stream=None, ws=None):
    """One C-ABI call form of a side library -> (status, costs, grads or None).  form: one | two | inplace | score | host, and
    the halves of `two` on their own, fwd | bwd.  one(grads_ptr or None, costs_ptr, ws_ptr), fwd(costs_ptr, ws_ptr) and
    bwd(grads_ptr, scale_ptr or None, ws_ptr) call the library's three entries with its own arguments around these.  Costs and
    gradients start as NaN; `host` hands the entry a host array for the costs, `inplace` the logits for the gradients, `score`
    no gradients.  ws: the caller's workspace (anything with a data_ptr(), of ws_bytes bytes or more) in place of a fresh
    torch.empty: tests/ws_contract.py plants its contents and its guards."""
    N = x.shape[0]
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    costs = torch.full((N,), float("nan"), dtype=cdt, device=DEV)
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    if grads is None and form not in ("score", "inplace", "host", "fwd"):
        grads = torch.full_like(x, float("nan"))
    if form in ("one", "score", "inplace", "host"):
        g = None if form == "score" else (x if form == "inplace" else grads)
        gp = g.data_ptr() if g is not None else None
        if form == "host":
            hc = np.full(N, np.nan, dtype=np.float64 if cdt == torch.float64 else np.float32)
            st = one(gp, hc.ctypes.data, ws.data_ptr())
            return st, hc, (None if g is None else g.double().cpu().numpy())
        st = one(gp, costs.data_ptr(), ws.data_ptr())
        (stream or torch.cuda.current_stream()).synchronize()
        return st, costs.cpu().numpy(), (None if g is None else g.double().cpu().numpy())
    if form != "bwd":
        st = fwd(costs.data_ptr(), ws.data_ptr())
        assert st == 0
        if form == "fwd":
            torch.cuda.synchronize()
            return st, costs.cpu().numpy(), None
    sc = None if scale is None else torch.tensor(scale, dtype=cdt, device=DEV)
    st = bwd(grads.data_ptr(), sc.data_ptr() if sc is not None else None, ws.data_ptr())
    torch.cuda.synchronize()
    return st, (None if form == "bwd" else costs.cpu().numpy()), grads.double().cpu().numpy()
