#!/usr/bin/env python
"""Time the fused joiner (libwarprnnt_joiner.so, warprnnt_pytorch.joiner) beside the torch routes the tree had before it, on the
same f (N, T, H) and g (N, U, H) in the same process, forward + backward (the incoming gradient is a fixed tensor).
  fused_padded / torch_padded   joiner_padded              / act(f[:, :, None] + g[:, None])
  fused_packed / torch_packed   joiner_packed(rows, validate=False) / pack_joint of the padded tensor (its host loop included)
  fused_pruned / torch_pruned   joiner_pruned(validate=False) / act(am_p + lm_p) of prune_inputs
The torch route is timed before AND after the fused one (both values and their mean are reported); each route's peak device
memory (torch.cuda.max_memory_allocated over its steps, inputs included) is reported beside it.
Shapes, lengths spread evenly over [max / 2, max] (sample 0 full): c3 (N=128, T=150, U=21, H=512), long (N=16, T=375, U=101,
H=512), pruned (N=64, T=375, U=101, S=5, H=512), each in fp32 and bf16 with tanh and relu.  Each line: mean ms per step over
--steps (after --warmup) or as many more as fill --window seconds, one device synchronisation per step; the device time of
each kernel of the fused route (torch.profiler, mean over a few steps, in a TRACED pass of its own behind the timed steps); and
the fraction of the 8 TB/s HBM roofline the kernels reach on their algorithmic bytes: the forward, out written once (the real
rows and, padded, the zero rows); the backward, dout and out read once over the real rows (dout alone for identity), df and dg
written.  Run it in three processes and take medians.
Usage: python tools/joiner_bench.py [--steps K] [--warmup W] [--window S] [--config c3_f32_tanh ...]"""
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
SHAPES = {"c3": (128, 150, 21, 512, 0), "long": (16, 375, 101, 512, 0), "pruned": (64, 375, 101, 512, 5)}
CONFIGS = {"%s_%s_%s" % (s, d, a): (s, dt, a) for s in SHAPES for d, dt in (("f32", torch.float32), ("bf16", torch.bfloat16))
           for a in ("tanh", "relu")}
KERNELS = ("joiner_prep_kernel", "joiner_fwd_kernel", "joiner_bwd_kernel", "joiner_dg_sum_kernel", "joiner_df_kernel",
           "joiner_dg_kernel")
ACT = {"tanh": torch.tanh, "relu": torch.relu}


def timed(fn, steps, warmup, window_s):
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


def measured(fn, steps, warmup, window_s, dev):
    """(ms per step, peak bytes allocated over the steps)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = timed(fn, steps, warmup, window_s)
    return ms, torch.cuda.max_memory_allocated(dev)


def kernel_us(fn, reps=5):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            for k in KERNELS:
                if ("::" + k + "<") in e.name:
                    out[k] = out.get(k, 0.0) + e.device_time / reps
    return out


def spread(n, top, low, dev):
    """n int32 lengths spread evenly over [low, top], the first one top."""
    return torch.linspace(top, low, n, device=dev).round().to(torch.int32)


def diagonal_windows(tl, ll, T, S, U, dev):
    """(N, T) int32 starts around the diagonal u = t L_b / T_b of each sample, clamped to [0, max(0, L_b + 1 - S)]."""
    t = torch.arange(T, device=dev, dtype=torch.float64)[None, :]
    s = torch.round(t * ll[:, None] / tl[:, None]) - S // 2
    return torch.minimum(s.clamp(min=0), (ll[:, None] + 1 - S).clamp(min=0).double()).to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS))
    a = ap.parse_args()
    from warprnnt_pytorch import joiner
    from warprnnt_pytorch.packed import pack_joint, row_offsets
    from warprnnt_pytorch.pruned import prune_inputs
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        shape, dt, act = CONFIGS[cfg]
        N, T, U, H, S = SHAPES[shape]
        esz = torch.finfo(dt).bits // 8
        f = torch.randn((N, T, H), generator=gen, device=dev).to(dt).requires_grad_(True)
        g = torch.randn((N, U, H), generator=gen, device=dev).to(dt).requires_grad_(True)
        tl, ll = spread(N, T, T // 2, dev), spread(N, U - 1, (U - 1) // 2, dev)
        routes = {}
        if S:
            ranges = diagonal_windows(tl, ll, T, S, U, dev)
            dout = torch.randn((N, T, S, H), generator=gen, device=dev).to(dt)
            real_rows, all_rows = int(tl.sum()) * S, N * T * S
            routes["pruned"] = (lambda: joiner.joiner_pruned(f, g, ranges, S, tl, act, validate=False),
                                lambda: ACT[act](torch.add(*prune_inputs(f, g, ranges, S))), dout, all_rows)
        else:
            offsets = row_offsets(tl, ll)
            R = int(offsets[-1])
            real_rows = R
            routes["padded"] = (lambda: joiner.joiner_padded(f, g, tl, ll, act, validate=False),
                                lambda: ACT[act](f[:, :, None] + g[:, None]),
                                torch.randn((N, T, U, H), generator=gen, device=dev).to(dt), N * T * U)
            routes["packed"] = (lambda: joiner.joiner_packed(f, g, tl, ll, act, offsets=offsets, rows=R, validate=False),
                                lambda: pack_joint(ACT[act](f[:, :, None] + g[:, None]), tl, ll),
                                torch.randn((R, H), generator=gen, device=dev).to(dt), R)

        def step(route, d):
            def fn():
                f.grad = g.grad = None
                route().backward(d)
            return fn

        line = {"config": cfg, "dtype": str(dt).split(".")[-1], "act": act, "N": N, "T": T, "U": U, "S": S, "H": H,
                "real_rows": real_rows, "routes": {}}
        for name, (fused, torch_route, d, written_rows) in routes.items():
            before, peak_t = measured(step(torch_route, d), a.steps, a.warmup, a.window, dev)
            ms, peak = measured(step(fused, d), a.steps, a.warmup, a.window, dev)
            after, peak_t2 = measured(step(torch_route, d), a.steps, a.warmup, a.window, dev)
            us = kernel_us(step(fused, d))
            row = H * esz
            fwd_bytes = written_rows * row
            bwd_bytes = 2 * real_rows * row + (N * T + N * U) * row                 # dout and out read; df and dg written
            fwd_us = us.get("joiner_fwd_kernel", 0.0)
            bwd_us = sum(v for k, v in us.items() if k not in ("joiner_fwd_kernel", "joiner_prep_kernel"))

            def frac(nbytes, t):
                return round(nbytes / (t * 1e-6) / 1e9 / HBM_GBS, 3) if t > 0 else None
            torch_ms = 0.5 * (before + after)
            line["routes"][name] = {"fused_ms": round(ms, 4), "torch_ms": round(torch_ms, 4), "torch_before_ms": round(before, 4),
                                    "torch_after_ms": round(after, 4), "torch_over_fused": round(torch_ms / ms, 3),
                                    "fused_peak_mb": round(peak / 2 ** 20, 1), "torch_peak_mb": round(max(peak_t, peak_t2) / 2 ** 20, 1),
                                    "out_mb": round(written_rows * row / 2 ** 20, 1),
                                    "kernel_us": {k: round(v, 1) for k, v in us.items()},
                                    "hbm_frac": {"fwd": frac(fwd_bytes, fwd_us), "bwd": frac(bwd_bytes, bwd_us)}}
            del d
        print(json.dumps(line), flush=True)
        del f, g, routes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
