#!/usr/bin/env python
"""Time the TDT best-path alignment (libwarprnnt_tdt_align.so) beside the score-only TDT loss (libwarprnnt_tdt.so,
compute_tdt_loss_fwd with prepare_backward = 0) on the same tensors, in the same process, through the C-ABI.
  loss  : statistics + the loss's lattice (forward and backward sweeps, a block each)
  align : statistics + the max-plus lattice with back-pointers + the traceback
Shapes: c3 (N=128, T=150, U=21, A=5000+5, fp32), c5 (N=128, T=200, U=41, A=1024+5, bf16) and `long` (N=2, T=1500, U=301, A=3+5,
fp32: the traceback's serial walk of T_b + L_b = 1800 steps).  Each line: mean ms per call over --steps (after --warmup), one
device synchronisation per call; per-kernel device times (torch.profiler, mean over a few calls); the alignment without its
traceback against the loss; and the traceback's time per step of the longest sample.
Usage: python tools/tdt_align_bench.py [--steps K] [--warmup W] [--config c3 c5 long]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
    sys.path.insert(0, p)
import torch

DURATIONS = (0, 1, 2, 3, 4)
CONFIGS = {"c3": (128, 150, 21, 5000, torch.float32), "c5": (128, 200, 41, 1024, torch.bfloat16),
           "long": (2, 1500, 301, 3, torch.float32)}
KERNELS = ["tdt_stats_kernel", "tdt_lattice_kernel", "tdt_align_lattice_kernel", "tdt_align_traceback_kernel"]


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
            if n + "<" in e.name or "%d%sI" % (len(n), n) in e.name:          # demangled, or the mangled template name
                out[n] += e.device_time / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["c3", "c5", "long"])
    a = ap.parse_args()
    from warprnnt_pytorch import _side, tdt, tdt_align
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    D = len(DURATIONS)
    dur = (C.c_int * D)(*DURATIONS)
    for cfg in a.config:
        N, T, U, A, dt = CONFIGS[cfg]
        code = _side.DT[dt]
        labels = torch.randint(0, A - 1, (N, U - 1), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), U - 1, dtype=torch.int32, device=dev)
        acts = torch.randn((N, T, U, A + D), generator=gen, device=dev).to(dt)
        costs = torch.empty(N, dtype=torch.float32, device=dev)
        score = torch.empty(N, dtype=torch.float64, device=dev)
        frames = torch.empty((N, U - 1), dtype=torch.int32, device=dev)
        durs = torch.empty((N, U - 1), dtype=torch.int32, device=dev)
        ws_loss = torch.empty(tdt.workspace_bytes(T, U, N, D, code), dtype=torch.uint8, device=dev)
        ws_align = torch.empty(tdt_align.workspace_bytes(T, U, N, D, code), dtype=torch.uint8, device=dev)
        opt = _side.options(dev, A - 1, T, U)
        lens = (labels.data_ptr(), label_lens.data_ptr(), act_lens.data_ptr(), A, N)

        def loss():
            st = tdt.lib().compute_tdt_loss_fwd(acts.data_ptr(), dur, D, 0.0, *lens, costs.data_ptr(), ws_loss.data_ptr(), opt,
                                                code, 0)
            assert st == 0

        def align():
            st = tdt_align.lib().compute_tdt_align(acts.data_ptr(), dur, D, 0.0, *lens, score.data_ptr(), frames.data_ptr(),
                                                   durs.data_ptr(), ws_align.data_ptr(), opt, code)
            assert st == 0

        ms_loss = timed(loss, a.steps, a.warmup)
        ms_align = timed(align, a.steps, a.warmup)
        kl = kernel_us(loss, KERNELS)
        ka = kernel_us(align, KERNELS)
        assert torch.isfinite(score).all() and bool((score <= -costs.double() + 1e-3).all())
        sweep = ka["tdt_stats_kernel"] + ka["tdt_align_lattice_kernel"]
        full = kl["tdt_stats_kernel"] + kl["tdt_lattice_kernel"]
        tb = ka["tdt_align_traceback_kernel"]
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A,
                          "durations": list(DURATIONS), "loss_score_only_ms": round(ms_loss, 4), "align_ms": round(ms_align, 4),
                          "loss_kernels_us": {n: round(v, 1) for n, v in kl.items() if v > 0},
                          "align_kernels_us": {n: round(v, 1) for n, v in ka.items() if v > 0},
                          "align_without_traceback_us": round(sweep, 1), "loss_kernels_total_us": round(full, 1),
                          "align_without_traceback_vs_loss": round(sweep / full, 3) if full > 0 else None,
                          "traceback_us": round(tb, 1), "traceback_steps": T + U - 1,
                          "traceback_ns_per_step": round(tb * 1e3 / (T + U - 1), 1)}), flush=True)
        del acts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
