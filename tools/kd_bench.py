#!/usr/bin/env python
"""Time the transducer lattice distillation loss (libwarprnnt_kd.so) beside the same loss in plain torch on the same
tensors, in the same process.
  module : TransducerKDLoss(reduction='mean') on (N, T, U, A) student and teacher logits, forward + backward (two phases)
  cabi   : compute_kd_loss, one call with device costs into preallocated gradients and workspace
  torch  : kd_loss_torch(...).backward() -- log_softmax of both tensors, gather, mask, autograd (the route this replaces)
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32), c5 (N=128, T=200, L=40, A=1024, bf16), c2 (N=16, T=150, L=40, A=28, fp32), both
modes.  Each line: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step (the torch route: --torch-steps, or a second's worth); the peak of torch.cuda.max_memory_allocated over a step of the module and of the torch route, beyond the
bytes the inputs hold (the gradient tensor counts on both routes); per-kernel times (torch.profiler device times, mean
over a few steps, in a TRACED pass of their own behind the timed steps: under the tracer a kernel can take a few per cent
longer than in the untraced call, so the stage fractions are lower bounds and the call's own fraction can exceed them); and
fractions of the 8 TB/s HBM roofline on the byte model -- E = bytes of one logits tensor; statistics 2 E (both tensors read once), gradient stream 2 E collapsed (student read, gradient written) or 3 E full, the call 4 E / 5 E.
Usage: python tools/kd_bench.py [--steps K] [--warmup W] [--torch-steps K] [--config c3 c5 c2] [--mode collapsed full]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
    sys.path.insert(0, p)
import torch

HBM_GBS = 8000.0
CONFIGS = {"c3": (128, 150, 20, 5000, torch.float32), "c5": (128, 200, 40, 1024, torch.bfloat16),
           "c2": (16, 150, 40, 28, torch.float32)}
KERNELS = ["kd_stats_kernel", "kd_cost_kernel", "kd_grad_kernel", "kd_grad_elem_kernel"]


def timed(fn, steps, warmup, window_s=1.0):
    """Mean ms per step over at least `steps` steps and at least `window_s` seconds (the step count of a short step is
    raised from the time of the warm-up steps), one synchronisation per step."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
        torch.cuda.synchronize()
    steps = max(steps, min(20000, int(window_s / max((time.perf_counter() - t0) / 3, 1e-6)) + 1))
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def peak_extra_bytes(fn, clear):
    """Peak of the allocator over one step, beyond what the inputs hold (clear() drops the previous step's gradient)."""
    fn()
    torch.cuda.synchronize()
    clear()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def kernel_us(fn, names, reps=5):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {n: 0.0 for n in names}
    for e in prof.events():
        if e.device_type != DeviceType.CUDA:
            continue
        for n in names:
            if n + "<" in e.name:
                out[n] += e.device_time / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["c3", "c5", "c2"])
    ap.add_argument("--mode", nargs="+", default=["collapsed", "full"])
    a = ap.parse_args()
    from warprnnt_pytorch import _side, kd
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        N, T, L, A, dt = CONFIGS[cfg]
        U = L + 1
        esz = torch.finfo(dt).bits // 8
        code = _side.DT[dt]
        labels = torch.randint(0, A - 1, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        acts = (torch.randn((N, T, U, A), generator=gen, device=dev) * 2).to(dt).requires_grad_(True)
        with torch.no_grad():
            teacher = (torch.randn((N, T, U, A), generator=gen, device=dev) * 2).to(dt)
        E = N * T * U * A * esz
        for mode in a.mode:
            tau = 2.0
            module = kd.TransducerKDLoss(blank=A - 1, mode=mode, temperature=tau, reduction="mean")

            def step_module():
                acts.grad = None
                module(acts, teacher, labels, act_lens, label_lens).backward()

            def step_torch():
                acts.grad = None
                kd.kd_loss_torch(acts, teacher, labels, act_lens, label_lens, A - 1, mode, tau, "mean").backward()

            grads = torch.empty_like(acts)
            costs = torch.empty(N, dtype=torch.float64 if dt == torch.float64 else torch.float32, device=dev)
            ws = torch.empty(kd.workspace_bytes(T, U, N, code), dtype=torch.uint8, device=dev)
            opt = _side.options(dev, A - 1, T, U)
            lib = kd.lib()

            def clear():
                acts.grad = None

            def step_cabi():
                st = lib.compute_kd_loss(acts.data_ptr(), teacher.data_ptr(), grads.data_ptr(), labels.data_ptr(),
                                         label_lens.data_ptr(), act_lens.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(), opt,
                                         code, kd.MODES[mode], ctypes.c_float(tau))
                assert st == 0, st

            ms = {"module": timed(step_module, a.steps, a.warmup), "cabi": timed(step_cabi, a.steps, a.warmup)}
            ku = kernel_us(step_cabi, KERNELS)
            del grads, ws
            acts.grad = None
            mem = {"module": peak_extra_bytes(step_module, clear)}
            acts.grad = None
            ms["torch"] = timed(step_torch, a.torch_steps, 2)
            acts.grad = None
            mem["torch"] = peak_extra_bytes(step_torch, clear)
            acts.grad = None
            torch.cuda.empty_cache()
            model = (4 if mode == "collapsed" else 5) * E
            frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
            gk = ku["kd_grad_kernel"] + ku["kd_grad_elem_kernel"]
            print(json.dumps({"config": cfg, "mode": mode, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A,
                              "temperature": tau, "logits_mb": round(E / 2 ** 20, 1),
                              "module_ms": round(ms["module"], 4), "cabi_ms": round(ms["cabi"], 4),
                              "torch_ms": round(ms["torch"], 4),
                              "module_vs_torch_time": round(ms["module"] / ms["torch"], 4),
                              "module_peak_mb": round(mem["module"] / 2 ** 20, 1), "torch_peak_mb": round(mem["torch"] / 2 ** 20, 1),
                              "module_vs_torch_peak": round(mem["module"] / mem["torch"], 4),
                              "kernels_us": {n: round(v, 1) for n, v in ku.items() if v > 0},
                              "stats_hbm_frac": frac(2 * E, ku["kd_stats_kernel"]),
                              "grad_hbm_frac": frac((2 if mode == "collapsed" else 3) * E, gk),
                              "cabi_hbm_frac": frac(model, ms["cabi"] * 1e3),
                              "module_hbm_frac": frac(model, ms["module"] * 1e3)}), flush=True)
        del acts, teacher
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
