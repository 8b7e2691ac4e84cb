#!/usr/bin/env python
"""Time the prune ranges from occupations and the window coverage (libwarprnnt_ranges.so, warprnnt_pytorch.ranges) beside
yardsticks that are not the code under test, at the lattice shapes of c4 (B=64, T=1500, S=300), c3 (B=128, T=150, S=20) and
c2 (B=16, T=150, S=40), window width 5, regular and modified type, fp32 and bf16.  Per shape, type and dtype:
  (a) ranges   : prune_ranges_from_occupations, wall ms per call, and the device time of its two kernels
  (b) coverage : range_coverage on those ranges, wall ms per call, and its kernel's device time
  (c) torch    : the plain-torch formulation on the same tensors -- g = py + pad(px), pad, cumsum over (B, S + 2, T), two
                 slices, argmax, the clamp and the two monotone passes as cummax -- wall ms per call, and how many of its
                 starts equal the library's (its cumsum adds in the backend's order: near-ties may differ)
  (d) mi       : the mutual_information_recursion(px, py, return_grad=True) call that produces such occupations
  (e) roofline : the algorithmic traffic -- one read of both arrays -- over the window kernel's device time, as a fraction of
                 the HBM rate of --hbm-tbs (6.29 TB/s measured copy rate by default)
Each wall time: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step; device times from torch.profiler, mean over a few steps, in a traced pass of its own.

Without --child this process never touches the GPU: it starts one child process per run and shape, each under a time limit
of its own (--limit seconds), three runs by default, stops at the first child that fails or runs out of time, and writes run
K's lines to <out>/ranges_bench_runK.jsonl (profiles/ranges by default).
Usage: python tools/ranges_bench.py [--runs 3] [--steps K] [--warmup W] [--config c4 c3 c2] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c4": (64, 1500, 300), "c3": (128, 150, 20), "c2": (16, 150, 40)}
R = 5
STAGES = {"window": ["ranges_window_kernel"], "repair": ["ranges_repair_kernel"], "coverage": ["ranges_coverage_kernel"]}


def child(a):
    for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
        sys.path.insert(0, p)
    import torch
    from warprnnt_pytorch import mi, ranges

    def timed(fn, steps, warmup, window_s=1.0):
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

    def stage_us(fn, reps=5):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {s: 0.0 for s in STAGES}
        for e in prof.events():
            if e.device_type != DeviceType.CUDA:
                continue
            for s, names in STAGES.items():
                if any(n in e.name for n in names):            # (demangled or not)
                    out[s] += e.device_time / reps
        return {k: round(v, 1) for k, v in out.items() if v}

    def torch_ranges(gx, gy, step):
        """The plain-torch formulation, full rectangle: starts (B, T) int64."""
        B, S1, T = gy.shape
        S = S1 - 1
        g = gy.to(torch.float64, copy=True)
        g[:, :S] += gx.double()[:, :, :T]
        c = torch.nn.functional.pad(g, (0, 0, 1, 0)).cumsum(1)                       # (B, S + 2, T)
        smax = S + 1 - R
        w = c[:, R:R + smax + 1] - c[:, :smax + 1]
        s = w.argmax(1)                                                              # (B, T)
        t = torch.arange(T, device=g.device)
        lo, hi = (smax - (T - 1 - t) * step).clamp(min=0), (t * step).clamp(max=smax)
        s = torch.minimum(torch.maximum(s, lo), hi).cummax(1).values
        return (s - t * step).flip(1).cummax(1).values.flip(1) + t * step

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cfg = a.child
    B, T, S = CONFIGS[cfg]
    base_x = torch.rand((B, S, T + 1), generator=gen, device=dev) * -3.0
    base_y = torch.rand((B, S + 1, T), generator=gen, device=dev) * -3.0
    ranges.lib()
    for dtype in (torch.float32, torch.bfloat16):
        for mod in (0, 1):
            xd = (base_x[:, :, :T] if mod else base_x).to(dtype).contiguous()
            yd = base_y.to(dtype).contiguous()
            _, (gx, gy) = mi.mutual_information_recursion(xd, yd, return_grad=True)
            step = 1 if mod else R - 1
            holder = {}

            def step_ranges():
                holder["s"] = ranges.prune_ranges_from_occupations(gx, gy, None, R, validate=False)

            def step_coverage():
                holder["k"] = ranges.range_coverage(gx, gy, holder["s"], R, validate=False)

            def step_mi():
                mi.mutual_information_recursion(xd, yd, return_grad=True, validate=False)

            line = {"config": cfg, "dtype": str(dtype).split(".")[-1], "type": "modified" if mod else "regular", "B": B, "T": T,
                    "S": S, "R": R, "step": step}
            line["ranges_ms"] = round(timed(step_ranges, a.steps, a.warmup), 4)
            line["coverage_ms"] = round(timed(step_coverage, a.steps, a.warmup), 4)
            line["mi_fwd_bwd_ms"] = round(timed(step_mi, a.steps, a.warmup), 4)
            us = stage_us(lambda: (step_ranges(), step_coverage()))
            line["window_us"], line["repair_us"], line["coverage_us"] = us.get("window"), us.get("repair"), us.get("coverage")
            want = torch_ranges(gx, gy, step)
            line["torch_ms"] = round(timed(lambda: torch_ranges(gx, gy, step), a.steps, 2), 4)
            line["torch_agrees"] = round((want == holder["s"]).double().mean().item(), 6)
            line["mean_kept"] = round(holder["k"].mean().item(), 6)
            line["torch_over_ranges"] = round(line["torch_ms"] / line["ranges_ms"], 1)
            line["ranges_over_mi"] = round(line["ranges_ms"] / line["mi_fwd_bwd_ms"], 4)
            nbytes = (gx.numel() - (0 if mod else B * S) + gy.numel()) * gx.element_size()   # (column T of px is not read)
            line["algorithmic_MB"] = round(nbytes / 1e6, 2)
            for k in ("window", "coverage"):
                if us.get(k):
                    line[k + "_TBs"] = round(nbytes / (us[k] * 1e-6) / 1e12, 3)
                    line[k + "_hbm_fraction"] = round(line[k + "_TBs"] / a.hbm_tbs, 3)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="the HBM rate the roofline fraction is taken of, TB/s")
    ap.add_argument("--config", nargs="+", default=["c4", "c3", "c2"])
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranges"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for run in range(1, a.runs + 1):
        path = os.path.join(a.out, "ranges_bench_run%d.jsonl" % run)
        with open(path, "w") as f:
            for cfg in a.config:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--steps", str(a.steps), "--warmup",
                       str(a.warmup), "--hbm-tbs", str(a.hbm_tbs)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    print("run %d %s: no result within %.0f s; stopping" % (run, cfg, a.limit), flush=True)
                    return 1
                if r.returncode != 0:
                    print("run %d %s: exit status %d; stopping\n%s" % (run, cfg, r.returncode, r.stderr[-2000:]), flush=True)
                    return 1
                for line in r.stdout.strip().splitlines():
                    if line.startswith("{"):
                        f.write(line + "\n")
                        print("run %d %s" % (run, line), flush=True)
                f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
