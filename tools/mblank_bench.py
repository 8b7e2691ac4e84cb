#!/usr/bin/env python
"""Time the multi-blank loss (libwarprnnt_mblank.so) beside RNNTLoss on the same tensor, in the same process.
  rnnt   : RNNTLoss(reduction='mean') on (N, T, U, A) logits, forward + backward
  mblank : MultiBlankLoss([2, 4, 8], blank=A - 1, reduction='mean') -- K = 3, NeMo's column layout -- on the same logits
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32) and c5 (N=128, T=200, L=40, A=1024, bf16).  Each line: mean ms per step over
--steps (after --warmup), one device synchronisation per step; the ratio mblank / rnnt; per-kernel times of the multi-blank
call (torch.profiler device times, mean over a few steps); and the fraction of the 8 TB/s HBM roofline the call reaches,
counted as one read (statistics) plus one read and one write (gradient) of the logits -- all rows lie inside the lattice here.
Usage: python tools/mblank_bench.py [--steps K] [--warmup W] [--config c3 c5]"""
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
DURATIONS = (2, 4, 8)
CONFIGS = {"c3": (128, 150, 20, 5000, torch.float32), "c5": (128, 200, 40, 1024, torch.bfloat16)}
KERNELS = ["mblank_stats_kernel", "mblank_lattice_kernel", "mblank_coef_kernel", "mblank_grad_kernel"]


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
    ap.add_argument("--config", nargs="+", default=["c3", "c5"])
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.mblank import MultiBlankLoss
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        N, T, L, A, dt = CONFIGS[cfg]
        U = L + 1
        K = len(DURATIONS)
        esz = torch.finfo(dt).bits // 8
        labels = torch.randint(0, A - 1 - K, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        acts = torch.rand((N, T, U, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        crit = RNNTLoss(blank=A - 1, reduction="mean")
        mcrit = MultiBlankLoss(DURATIONS, blank=A - 1, reduction="mean")

        def rnnt():
            acts.grad = None
            crit(acts, labels, act_lens, label_lens).backward()

        def mblank():
            acts.grad = None
            mcrit(acts, labels, act_lens, label_lens).backward()

        ms_rnnt = timed(rnnt, a.steps, a.warmup)
        ms = timed(mblank, a.steps, a.warmup)
        k = kernel_us(mblank, KERNELS)
        row_bytes = N * T * U * A * esz
        frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A,
                          "durations": list(DURATIONS), "rnnt_ms": round(ms_rnnt, 4), "mblank_ms": round(ms, 4),
                          "mblank_vs_rnnt": round(ms / ms_rnnt, 3), "logits_mb": round(row_bytes / 2 ** 20, 1),
                          "kernels_us": {n: round(v, 1) for n, v in k.items() if v > 0},
                          "stats_hbm_frac": frac(row_bytes, k["mblank_stats_kernel"]),
                          "grad_hbm_frac": frac(2 * row_bytes, k["mblank_grad_kernel"]),
                          "call_hbm_frac": frac(3 * row_bytes, ms * 1e3)}), flush=True)
        del acts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
