#!/usr/bin/env python
"""Time the HAT loss (libwarprnnt_hat.so) beside RNNTLoss and beside the route it replaces, on the same N, T, U, A.
  rnnt      : RNNTLoss(reduction='mean') on (N, T, U, A) logits, forward + backward
  hat       : HATLoss(reduction='mean') on the same logits, forward + backward
  composite : RNNTLoss(hat_log_probs(logits)) with autograd through the transform -- HAT without this library
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32), c5 (N=128, T=200, L=40, A=1024, bf16) and c4 (N=64, T=1500, L=300, A=50,
fp32), blank in column 0.  Each line: mean ms per step over --steps (after --warmup), one device synchronisation per step;
torch.cuda.max_memory_allocated of the hat and composite routes; and per-kernel times of the HAT call (torch.profiler device
times, mean over a few steps) with the streaming kernels' fraction of the 8 TB/s HBM roofline (statistics: every row read
once; gradient: every row read and written; all rows lie inside the lattice here).
Usage: python tools/hat_bench.py [--steps K] [--warmup W] [--config c3 c5 c4]"""
import argparse
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
           "c4": (64, 1500, 300, 50, torch.float32)}
KERNELS = ["hat_stats_kernel", "lattice_kernel", "lattice_lin_kernel", "coef_kernel", "coef_cell_kernel", "hat_grad_kernel"]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["c3", "c5", "c4"])
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.hat import HATLoss, hat_log_probs
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        N, T, L, A, dt = CONFIGS[cfg]
        U = L + 1
        esz = torch.finfo(dt).bits // 8
        labels = torch.randint(1, A, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        acts = torch.rand((N, T, U, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        crit, hcrit = RNNTLoss(reduction="mean"), HATLoss(blank=0, reduction="mean")

        def rnnt():
            acts.grad = None
            crit(acts, labels, act_lens, label_lens).backward()

        def hat():
            acts.grad = None
            hcrit(acts, labels, act_lens, label_lens).backward()

        def composite():
            acts.grad = None
            crit(hat_log_probs(acts, 0), labels, act_lens, label_lens).backward()

        ms_rnnt = timed(rnnt, a.steps, a.warmup)
        ms = timed(hat, a.steps, a.warmup)
        k = kernel_us(hat, KERNELS)
        mem_hat = peak_mb(hat)
        ms_comp = timed(composite, a.steps, a.warmup)
        mem_comp = peak_mb(composite)
        row_bytes = N * T * U * A * esz
        frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A,
                          "rnnt_ms": round(ms_rnnt, 4), "hat_ms": round(ms, 4), "composite_ms": round(ms_comp, 4),
                          "hat_vs_rnnt": round(ms / ms_rnnt, 3), "composite_vs_hat": round(ms_comp / ms, 3),
                          "logits_mb": round(row_bytes / 2 ** 20, 1), "hat_peak_mb": mem_hat, "composite_peak_mb": mem_comp,
                          "kernels_us": {n: round(v, 1) for n, v in k.items() if v > 0},
                          "stats_hbm_frac": frac(row_bytes, k["hat_stats_kernel"]),
                          "grad_hbm_frac": frac(2 * row_bytes, k["hat_grad_kernel"])}), flush=True)
        del acts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
