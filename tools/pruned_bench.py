#!/usr/bin/env python
"""Time the pruned loss (libwarprnnt_pruned.so) against the materialised call on the c3 shape (N=128, T=150, L=20, A=5000).
  materialised : RNNTLoss(reduction='mean') on (N, T, L + 1, A) logits, forward + backward (what bench.py times)
  pruned S     : rnnt_loss_pruned(reduction='mean') on (N, T, S, A) logits, forward + backward, for S in {4, 8}
  ranges       : prune_ranges(f, g, S) on the additive joint f (N, T, A), g (N, L + 1, A)
Each line: mean ms per step over --steps (after --warmup), one device synchronisation per step, and for the pruned rows the two
streaming kernels' times (torch.profiler, mean over a few steps) with their fraction of the 8 TB/s HBM roofline
(statistics: the in-lattice rows read once; gradient: every row written, the in-lattice rows also read).
Usage: python tools/pruned_bench.py [--steps K] [--warmup W] [--dtype fp32|bf16 ...]"""
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
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_us(fn, prefixes, reps=5):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {p: 0.0 for p in prefixes}
    for e in prof.events():
        if e.device_type != DeviceType.CUDA:
            continue
        for p in prefixes:
            if p in e.name:
                out[p] += e.device_time / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--shape", default="128,150,20,5000", help="N,T,L,A")
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch import pruned as P
    N, T, L, A = (int(x) for x in a.shape.split(","))
    U = L + 1
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    labels = torch.randint(1, A, (N, L), generator=gen, device=dev, dtype=torch.int32)
    act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
    label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
    for dname in a.dtype:
        dt = DT[dname]
        esz = torch.finfo(dt).bits // 8
        acts = torch.rand((N, T, U, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        crit = RNNTLoss(reduction="mean")

        def mat():
            acts.grad = None
            crit(acts, labels, act_lens, label_lens).backward()
        ms_mat = timed(mat, a.steps, a.warmup)
        print(json.dumps({"what": "materialised", "dtype": dname, "N": N, "T": T, "U": U, "A": A, "ms": round(ms_mat, 4)}))
        del acts, crit
        torch.cuda.empty_cache()
        f = torch.rand((N, T, A), generator=gen, device=dev).to(dt)
        g = torch.rand((N, U, A), generator=gen, device=dev).to(dt)
        for S in (4, 8):
            ranges = P.prune_ranges(f, g, labels, act_lens, label_lens, S)
            ms_r = timed(lambda: P.prune_ranges(f, g, labels, act_lens, label_lens, S), a.steps, a.warmup)
            x = torch.rand((N, T, S, A), generator=gen, device=dev).to(dt).requires_grad_(True)

            def step():
                x.grad = None
                P.rnnt_loss_pruned(x, labels, act_lens, label_lens, ranges, validate=False).backward()
            ms = timed(step, a.steps, a.warmup)
            k = kernel_us(step, ["pruned_stats_kernel", "pruned_grad_kernel"])
            inlat = int(((ranges.unsqueeze(-1) + torch.arange(S, device=dev)) <= L).sum())
            rows = N * T * S
            b_stats = inlat * A * esz
            b_grad = (rows + inlat) * A * esz
            frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
            print(json.dumps({"what": "pruned fwd+bwd", "dtype": dname, "S": S, "ms": round(ms, 4),
                              "vs_materialised": round(ms / ms_mat, 3), "prune_ranges_ms": round(ms_r, 4),
                              "stats_us": round(k["pruned_stats_kernel"], 1), "stats_hbm_frac": frac(b_stats, k["pruned_stats_kernel"]),
                              "grad_us": round(k["pruned_grad_kernel"], 1), "grad_hbm_frac": frac(b_grad, k["pruned_grad_kernel"])}))
            del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
