#!/usr/bin/env python
"""Time the TDT loss (libwarprnnt_tdt.so) beside RNNTLoss on the same N, T, U.
  rnnt : RNNTLoss(reduction='mean') on (N, T, U, A) logits, forward + backward
  tdt  : TDTLoss(durations, reduction='mean') on (N, T, U, A + D) logits, forward + backward
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32) and c5 (N=128, T=200, L=40, A=1025 tokens, bf16) by default, durations
[0, 1, 2, 3, 4].  Each line: mean ms per step over --steps (after --warmup), one device synchronisation per step, and per-kernel
times of the TDT call (torch.profiler, mean over a few steps) with the streaming kernels' fraction of the 8 TB/s HBM roofline
(statistics: every row read once; gradient: every row read and written; all rows lie inside the lattice here).
Usage: python tools/tdt_bench.py [--steps K] [--warmup W] [--config c3 c5]"""
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
CONFIGS = {"c3": (128, 150, 20, 5000, torch.float32), "c5": (128, 200, 40, 1025, torch.bfloat16)}
KERNELS = ["tdt_stats_kernel", "tdt_lattice_kernel", "tdt_coef_kernel", "tdt_grad_kernel"]


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
    ap.add_argument("--durations", default="0,1,2,3,4")
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.tdt import TDTLoss
    durs = tuple(int(d) for d in a.durations.split(","))
    D = len(durs)
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
        crit = RNNTLoss(reduction="mean")

        def rnnt():
            acts.grad = None
            crit(acts, labels, act_lens, label_lens).backward()
        ms_rnnt = timed(rnnt, a.steps, a.warmup)
        del acts
        torch.cuda.empty_cache()
        x = torch.rand((N, T, U, A + D), generator=gen, device=dev).to(dt).requires_grad_(True)
        tcrit = TDTLoss(durs, blank=A - 1, reduction="mean")

        def tdt():
            x.grad = None
            tcrit(x, labels, act_lens, label_lens).backward()
        ms = timed(tdt, a.steps, a.warmup)
        k = kernel_us(tdt, KERNELS)
        row_bytes = N * T * U * (A + D) * esz
        frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A, "D": D,
                          "rnnt_ms": round(ms_rnnt, 4), "tdt_ms": round(ms, 4), "tdt_vs_rnnt": round(ms / ms_rnnt, 3),
                          "kernels_us": {n: round(v, 1) for n, v in k.items()},
                          "stats_hbm_frac": frac(row_bytes, k["tdt_stats_kernel"]),
                          "grad_hbm_frac": frac(2 * row_bytes, k["tdt_grad_kernel"])}))
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
