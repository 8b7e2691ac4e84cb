#!/usr/bin/env python
"""Time the monotonic loss (libwarprnnt_mono.so) beside RNNTLoss and the K = 0 multi-blank loss on the same tensor, in the
same process.
  rnnt   : RNNTLoss(reduction='mean') on (N, T, U, A) logits, forward + backward
  mblank : MultiBlankLoss((), blank=A - 1, reduction='mean') -- no big blanks: the plain lattice through the side-library
           skeleton this loss shares (statistics stream, lattice, coefficients, gradient stream) -- the yardstick
  mono   : MonotonicRNNTLoss(blank=A - 1, reduction='mean')
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32), c5 (N=128, T=200, L=40, A=1024, bf16) and c2 (N=16, T=150, L=40, A=28, fp32:
the small shape, where the lattice stage dominates).  Each line: mean ms per step over --steps (after --warmup), one device synchronisation per step; per-kernel times of
the multi-blank and of the monotonic call (torch.profiler device times, mean over a few steps); and the fraction of the
8 TB/s HBM roofline the monotonic streams reach, counted over the BAND rows only -- (L + 1)(T - L) + L of the T (L + 1)
rows of a sample: one read (statistics), one read and one write (gradient); the gradient stream also writes zeros over
the rows outside the band, which `grad_hbm_frac_all_writes` adds.
Usage: python tools/mono_bench.py [--steps K] [--warmup W] [--config c3 c5 c2]"""
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
           "c2": (16, 150, 40, 28, torch.float32)}
MBLANK_KERNELS = ["mblank_stats_kernel", "mblank_lattice_kernel", "mblank_coef_kernel", "mblank_grad_kernel"]
MONO_KERNELS = ["mono_stats_kernel", "mono_lattice_wave_kernel", "mono_lattice_block_kernel", "mono_coef_kernel",
                "mblank_grad_kernel"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["c3", "c5", "c2"])
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.mblank import MultiBlankLoss
    from warprnnt_pytorch.mono import MonotonicRNNTLoss
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        N, T, L, A, dt = CONFIGS[cfg]
        U = L + 1
        esz = torch.finfo(dt).bits // 8
        labels = torch.randint(0, A - 1, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        acts = torch.rand((N, T, U, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        crits = {"rnnt": RNNTLoss(blank=A - 1, reduction="mean"), "mblank": MultiBlankLoss((), blank=A - 1, reduction="mean"),
                 "mono": MonotonicRNNTLoss(blank=A - 1, reduction="mean")}

        def step(name):
            def fn():
                acts.grad = None
                crits[name](acts, labels, act_lens, label_lens).backward()
            return fn

        ms = {name: timed(step(name), a.steps, a.warmup) for name in ("rnnt", "mblank", "mono")}
        kb = kernel_us(step("mblank"), MBLANK_KERNELS)
        km = kernel_us(step("mono"), MONO_KERNELS)
        all_bytes = N * T * U * A * esz
        band_rows = (L + 1) * (T - L) + L
        band_bytes = N * band_rows * A * esz
        frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A,
                          "rnnt_ms": round(ms["rnnt"], 4), "mblank_k0_ms": round(ms["mblank"], 4),
                          "mono_ms": round(ms["mono"], 4), "mono_vs_mblank_k0": round(ms["mono"] / ms["mblank"], 3),
                          "logits_mb": round(all_bytes / 2 ** 20, 1), "band_fraction": round(band_rows / (T * U), 4),
                          "mblank_kernels_us": {n: round(v, 1) for n, v in kb.items() if v > 0},
                          "mono_kernels_us": {n: round(v, 1) for n, v in km.items() if v > 0},
                          "stats_hbm_frac": frac(band_bytes, km["mono_stats_kernel"]),
                          "grad_hbm_frac": frac(2 * band_bytes, km["mblank_grad_kernel"]),
                          "grad_hbm_frac_all_writes": frac(band_bytes + all_bytes, km["mblank_grad_kernel"]),
                          "call_hbm_frac": frac(3 * band_bytes, ms["mono"] * 1e3)}), flush=True)
        del acts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
