#!/usr/bin/env python
"""Time the fused edge log-probabilities (libwarprnnt_logprobs.so, warprnnt_pytorch.logprobs), forward + backward, beside the
torch route they replace (tools/pstream_bench.py's `torch_mi` without the lattice): log_softmax,
gathers of the blank and label columns, permutes and a cat -- in the pruned form a scatter by the window starts -- with autograd
keeping the pieces.  Both routes get the same incoming gradients for px and py; no lattice runs.
Shapes: c3 (B=128, T=150, S=20, C=5000) joint, c4 (B=64, T=1500, S=300, C=50) joint and c3 pruned at K = 4, in fp32 and bf16.
Each line: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step; peak memory of either route over what was allocated before it; per-stage device times of the fused
route (torch.profiler, mean over a few steps, in a traced pass of its own behind the timed steps) and the fraction of the 8 TB/s
HBM roofline they reach on the counted bytes: the forward reads the real rows of the logits once, the backward reads them once
and writes the tensor once.

Without --child this process never touches the GPU: it starts one child process per run and shape, each under a time limit
of its own (--limit seconds), three runs by default, stops at the first child that fails or runs out of time, and writes run
K's lines to profiles/logprobs/logprobs_bench_runK.jsonl.
Usage: python tools/logprobs_bench.py [--runs 3] [--steps K] [--warmup W] [--config c3_f32 ...] [--limit SECONDS]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (B, T, S, C, dtype, K)
CONFIGS = {"c3_f32": (128, 150, 20, 5000, "float32", 0), "c3_bf16": (128, 150, 20, 5000, "bfloat16", 0),
           "c4_f32": (64, 1500, 300, 50, "float32", 0), "c4_bf16": (64, 1500, 300, 50, "bfloat16", 0),
           "c3_f32_k4": (128, 150, 20, 5000, "float32", 4), "c3_bf16_k4": (128, 150, 20, 5000, "bfloat16", 4)}
STAGES = {"lse": "logprobs_lse_kernel", "edges": "logprobs_edges_kernel", "grad": "logprobs_grad_kernel"}
HBM_GBS = 8000.0


def child(a):
    for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
        sys.path.insert(0, p)
    import torch
    from warprnnt_pytorch import logprobs

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
            if e.device_type == DeviceType.CUDA:
                for s, name in STAGES.items():
                    if ("::" + name + "<") in e.name:
                        out[s] += e.device_time / reps
        return out

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cfg = a.child
    B, T, S, C, dtname, K = CONFIGS[cfg]
    dt = getattr(torch, dtname)
    U, blank, Kp = S + 1, C - 1, (K if K else S + 1)
    symbols = torch.randint(0, C - 1, (B, S), generator=gen, device=dev, dtype=torch.int32)
    z = torch.rand((B, T, Kp, C), generator=gen, device=dev).to(dt).requires_grad_(True)
    gx = torch.randn((B, S, T + 1), generator=gen, device=dev)
    gy = torch.randn((B, U, T), generator=gen, device=dev)
    ranges = None
    if K:
        t = torch.arange(T, device=dev, dtype=torch.float64)
        ranges = (torch.round(t * S / T) - K // 2).clamp(0, U - K).to(torch.int32).unsqueeze(0).expand(B, T).contiguous()
        u = ranges.long().unsqueeze(-1) + torch.arange(K, device=dev)                    # (B, T, K), all <= S
        lab_at = torch.gather(symbols.long().unsqueeze(1).expand(B, T, S), 2, u.clamp(max=S - 1))

    def fused():
        if K:
            return logprobs.get_rnnt_logprobs_pruned(z, symbols, ranges, blank, validate=False)
        return logprobs.get_rnnt_logprobs_joint(z, symbols, blank, validate=False)

    def torch_route():
        lp = torch.log_softmax(z.float(), -1)
        ninf = torch.full((B, T, U), float("-inf"), device=dev)
        if K:
            pxv = torch.where(u < S, torch.gather(lp, 3, lab_at.unsqueeze(-1)).squeeze(-1), ninf[..., :K])
            py = ninf.scatter(2, u, lp[..., blank]).transpose(1, 2).contiguous()
            px = ninf.scatter(2, u, pxv)[..., :S].transpose(1, 2)
        else:
            py = lp[..., blank].transpose(1, 2).contiguous()
            px = torch.gather(lp[:, :, :S], 3, symbols.long().view(B, 1, S, 1).expand(B, T, S, 1)).squeeze(-1).transpose(1, 2)
        return torch.cat((px, ninf[:, :1, :S].transpose(1, 2)), 2).contiguous(), py

    def step(route):
        def fn():
            z.grad = None
            px, py = route()
            torch.autograd.backward([px, py], [gx, gy])
        return fn

    # the yardstick computes what the library computes, on this very tensor
    with torch.no_grad():
        (fx, fy), (tx, ty) = fused(), torch_route()
        for f, t_ in ((fx, tx), (fy, ty)):
            assert torch.equal(f == float("-inf"), t_ == float("-inf"))
            m = f != float("-inf")
            assert torch.allclose(f[m], t_[m], rtol=1e-4, atol=1e-4)
        del fx, fy, tx, ty
    ms, peak = {}, {}
    for name, route in (("fused", fused), ("torch", torch_route)):
        z.grad = None
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ms[name] = timed(step(route), a.steps, a.warmup)
        peak[name] = torch.cuda.max_memory_allocated(dev) - before
    su = stage_us(step(fused))
    z.grad = None
    nbytes = z.numel() * z.element_size()
    frac = lambda n, us: round(n / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None       # noqa: E731
    print(json.dumps({"config": cfg, "dtype": dtname, "B": B, "T": T, "S": S, "C": C, "K": K, "logits_bytes": nbytes,
                      "ms": {k: round(v, 4) for k, v in ms.items()},
                      "torch_over_fused": round(ms["torch"] / ms["fused"], 2),
                      "peak_bytes": peak, "peak_torch_over_fused": round(peak["torch"] / max(peak["fused"], 1), 2),
                      "stages_us": {k: round(v, 1) for k, v in su.items()},
                      "hbm_fraction": {"forward": frac(nbytes, su["lse"] + su["edges"]), "lse": frac(nbytes, su["lse"]),
                                       "backward": frac(2 * nbytes, su["grad"]),
                                       "step": frac(3 * nbytes, ms["fused"] * 1e3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS))
    ap.add_argument("--limit", type=float, default=150.0, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for run in range(1, a.runs + 1):
        path = os.path.join(a.out, "logprobs_bench_run%d.jsonl" % run)
        with open(path, "w") as f:
            for cfg in a.config:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--steps", str(a.steps), "--warmup", str(a.warmup)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    print("run %d %s: no result within %.0f s; stopping" % (run, cfg, a.limit), flush=True)
                    return 1
                if r.returncode != 0:
                    print("run %d %s: exit status %d; stopping\n%s" % (run, cfg, r.returncode, r.stderr[-2000:]), flush=True)
                    return 1
                line = r.stdout.strip().splitlines()[-1]
                f.write(line + "\n")
                f.flush()
                print("run %d %s" % (run, line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
