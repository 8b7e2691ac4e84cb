#!/usr/bin/env python
"""Time the alignment-restricted loss (libwarprnnt_ar.so) beside RNNTLoss and beside itself with unrestricted windows on the
same tensor, in the same process.
  rnnt      : RNNTLoss(reduction='mean') on (N, T, U, A) logits, forward + backward -- the main library, untouched
  ar        : AlignmentRestrictedRNNTLoss(blank=A - 1, reduction='mean') with windows of +-W frames around a sorted random
              alignment (W = 5; 20 at c4)
  ar_open   : the same call with unrestricted windows (every row is a band row)
  mblank    : per-kernel times only, MultiBlankLoss((), blank=A - 1): its K = 0 lattice kernel is the candidate this library's
              block form was measured against
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32), c5 (N=128, T=200, L=40, A=1024, bf16), c2 (N=16, T=150, L=40, A=28, fp32) and
c4 (N=64, T=1500, L=300, A=50, fp32: the block form).  Each line: mean ms per step over --steps (after --warmup), one device
synchronisation per step; per-kernel times of the restricted, the unrestricted and the multi-blank call (torch.profiler
device times, mean over a few steps, taken in passes of their own behind the timed steps); the band's share of the rows; the
byte model's ratio (1 + 2 share) / 3 next to the measured ar / ar_open; and the fraction of the 8 TB/s HBM roofline the
restricted call's streams reach, counted over the band rows (the gradient stream also writes zeros over the rows outside the
band, which `grad_hbm_frac_all_writes` adds).
Usage: python tools/ar_bench.py [--steps K] [--warmup W] [--config c3 c5 c2 c4]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

HBM_GBS = 8000.0
CONFIGS = {"c3": (128, 150, 20, 5000, torch.float32, 5), "c5": (128, 200, 40, 1024, torch.bfloat16, 5),
           "c2": (16, 150, 40, 28, torch.float32, 5), "c4": (64, 1500, 300, 50, torch.float32, 20)}
AR_KERNELS = ["ar_bounds_kernel", "ar_stats_kernel", "ar_lattice_wave_kernel", "ar_lattice_block_kernel", "ar_coef_kernel",
              "mblank_grad_kernel"]
MBLANK_KERNELS = ["mblank_stats_kernel", "mblank_lattice_kernel", "mblank_coef_kernel", "mblank_grad_kernel"]


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


def band_rows(T, L, lo, hi):
    """Rows inside the band, summed over the batch (include/rnnt_ar.h): e = prefix maximum of lo from 0, l = suffix minimum
    of hi from T - 1, rows of column u: l_u - e_u + 1."""
    N = lo.shape[0]
    e = np.maximum.accumulate(np.concatenate((np.zeros((N, 1), np.int64), lo), 1), 1)
    l = np.minimum.accumulate(np.concatenate((hi, np.full((N, 1), T - 1, np.int64)), 1)[:, ::-1], 1)[:, ::-1]
    return int(np.clip(l - e + 1, 0, None).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["c3", "c5", "c2", "c4"])
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.ar import AlignmentRestrictedRNNTLoss
    from warprnnt_pytorch.mblank import MultiBlankLoss
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    rng = np.random.default_rng(7)
    for cfg in a.config:
        N, T, L, A, dt, W = CONFIGS[cfg]
        U = L + 1
        esz = torch.finfo(dt).bits // 8
        labels = torch.randint(0, A - 1, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        align = np.sort(rng.integers(0, T, size=(N, L)), 1)
        lo, hi = align - W, align + W
        wins = {"ar": [torch.tensor(v, dtype=torch.int32, device=dev) for v in (lo, hi)],
                "ar_open": [torch.full((N, L), v, dtype=torch.int32, device=dev) for v in (0, T - 1)]}
        acts = torch.rand((N, T, U, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        rnnt = RNNTLoss(blank=A - 1, reduction="mean")
        ar = AlignmentRestrictedRNNTLoss(blank=A - 1, reduction="mean")
        mblank = MultiBlankLoss((), blank=A - 1, reduction="mean")

        def step(name):
            def fn():
                acts.grad = None
                if name == "rnnt":
                    loss = rnnt(acts, labels, act_lens, label_lens)
                elif name == "mblank":
                    loss = mblank(acts, labels, act_lens, label_lens)
                else:
                    loss = ar(acts, labels, act_lens, label_lens, *wins[name])
                loss.backward()
            return fn

        ms = {name: timed(step(name), a.steps, a.warmup) for name in ("rnnt", "ar", "ar_open")}
        ka = kernel_us(step("ar"), AR_KERNELS)
        ko = kernel_us(step("ar_open"), AR_KERNELS)
        kb = kernel_us(step("mblank"), MBLANK_KERNELS)
        all_bytes = N * T * U * A * esz
        share = band_rows(T, L, lo, hi) / (N * T * U)
        band_bytes = share * all_bytes
        frac = lambda b, us: round(b / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A, "window": W,
                          "rnnt_ms": round(ms["rnnt"], 4), "ar_ms": round(ms["ar"], 4), "ar_open_ms": round(ms["ar_open"], 4),
                          "ar_vs_rnnt": round(ms["ar"] / ms["rnnt"], 3), "ar_vs_ar_open": round(ms["ar"] / ms["ar_open"], 3),
                          "band_share": round(share, 4), "modelled_ratio": round((1 + 2 * share) / 3, 3),
                          "logits_mb": round(all_bytes / 2 ** 20, 1),
                          "ar_kernels_us": {n: round(v, 1) for n, v in ka.items() if v > 0},
                          "ar_open_kernels_us": {n: round(v, 1) for n, v in ko.items() if v > 0},
                          "mblank_k0_kernels_us": {n: round(v, 1) for n, v in kb.items() if v > 0},
                          "stats_hbm_frac": frac(band_bytes, ka["ar_stats_kernel"]),
                          "grad_hbm_frac": frac(2 * band_bytes, ka["mblank_grad_kernel"]),
                          "grad_hbm_frac_all_writes": frac(band_bytes + all_bytes, ka["mblank_grad_kernel"]),
                          "call_hbm_frac": frac(3 * band_bytes, ms["ar"] * 1e3)}), flush=True)
        del acts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
