#!/usr/bin/env python
"""Time the delay-penalized loss (libwarprnnt_delay.so) with and without the expected emission frames, beside the routes the
tree had before it, on the same tensor in the same process.
  module       : DelayPenalizedRNNTLoss(blank=A - 1, reduction='mean'), forward + backward (two phases)
  module_emit  : the same step and one expected_emit_frames call (a forward call of its own, outside autograd)
  cabi         : compute_rnnt_loss_delay, one call with device costs into preallocated gradients and workspace, emit_frames
                 NULL
  cabi_emit    : the same call with an emit_frames array
each at delay_penalty = 0 and 0.01 (the same kernels run: a difference beyond run-to-run spread would be a finding), and
  rnnt         : RNNTLoss(reduction='mean'), forward + backward -- the main library
  mblank_k0    : MultiBlankLoss((), blank=A - 1): the K = 0 route through a side library
  ar_open      : AlignmentRestrictedRNNTLoss with unrestricted windows: the same skeleton and lattice kernels, the yardstick
Shapes: c3 (N=128, T=150, L=20, A=5000, fp32), c5 (N=128, T=200, L=40, A=1024, bf16), c2 (N=16, T=150, L=40, A=28, fp32) and
c4 (N=64, T=1500, L=300, A=50, fp32: the block lattice, a thread per column in the emission kernel).  Each line: mean ms per
step over --steps (after --warmup) or as many more as fill a window of one second, one device synchronisation per step;
per-stage device times of the one call with emit_frames at 0.01 (torch.profiler, mean over a few steps, in a TRACED pass of
its own behind the timed steps: under the tracer a kernel can take a few per cent longer); the emission kernel's share of
the forward stages; and the fraction of the 8 TB/s HBM roofline the call reaches on 3 E bytes (logits read twice, gradient
written once).  Run it in three processes and take medians.
Usage: python tools/delay_bench.py [--steps K] [--warmup W] [--config c3 c5 c2 c4]"""
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
           "c2": (16, 150, 40, 28, torch.float32), "c4": (64, 1500, 300, 50, torch.float32)}
STAGES = {"stats": ["delay_stats_kernel"], "lattice": ["ar_lattice_wave_kernel", "ar_lattice_block_kernel"],
          "coef": ["delay_coef_kernel"], "emit": ["delay_emit_kernel"], "grad": ["mblank_grad_kernel", "mblank_grad_elem_kernel"]}
PENALTIES = (0.0, 0.01)


def timed(fn, steps, warmup, window_s=1.0):
    """Mean ms per step over at least `steps` steps and at least `window_s` seconds (the step count of a short step is
    raised from the time of the warm-up steps), one synchronisation per step."""
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
            if any(n + "<" in e.name for n in names):
                out[s] += e.device_time / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=["c3", "c5", "c2", "c4"])
    a = ap.parse_args()
    from warprnnt_pytorch import RNNTLoss, _side, delay
    from warprnnt_pytorch.ar import AlignmentRestrictedRNNTLoss
    from warprnnt_pytorch.mblank import MultiBlankLoss
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        N, T, L, A, dt = CONFIGS[cfg]
        U = L + 1
        esz = torch.finfo(dt).bits // 8
        code = _side.DT[dt]
        labels = torch.randint(0, A - 1, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        open_lo, open_hi = (torch.full((N, L), v, dtype=torch.int32, device=dev) for v in (0, T - 1))
        acts = torch.rand((N, T, U, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        parents = {"rnnt": lambda m=RNNTLoss(blank=A - 1, reduction="mean"): m(acts, labels, act_lens, label_lens),
                   "mblank_k0": lambda m=MultiBlankLoss((), blank=A - 1, reduction="mean"): m(acts, labels, act_lens, label_lens),
                   "ar_open": lambda m=AlignmentRestrictedRNNTLoss(blank=A - 1, reduction="mean"):
                       m(acts, labels, act_lens, label_lens, open_lo, open_hi)}

        def step_parent(name):
            def fn():
                acts.grad = None
                parents[name]().backward()
            return fn

        def step_module(pen, emit):
            module = delay.DelayPenalizedRNNTLoss(blank=A - 1, delay_penalty=pen, reduction="mean")

            def fn():
                acts.grad = None
                module(acts, labels, act_lens, label_lens).backward()
                if emit:
                    delay.expected_emit_frames(acts, labels, act_lens, label_lens, A - 1, pen, validate=False)
            return fn

        ms = {name: timed(step_parent(name), a.steps, a.warmup) for name in parents}
        for pen in PENALTIES:
            for emit in (False, True):
                ms["module%s_p%g" % ("_emit" if emit else "", pen)] = timed(step_module(pen, emit), a.steps, a.warmup)
        acts.grad = None
        cdt = torch.float64 if dt == torch.float64 else torch.float32
        grads = torch.empty_like(acts)
        costs = torch.empty(N, dtype=cdt, device=dev)
        frames = torch.empty((N, L), dtype=cdt, device=dev)
        ws = torch.empty(delay.workspace_bytes(T, U, N, code), dtype=torch.uint8, device=dev)
        opt = _side.options(dev, A - 1, T, U)
        lib = delay.lib()

        def step_cabi(pen, emit):
            def fn():
                st = lib.compute_rnnt_loss_delay(acts.data_ptr(), pen, grads.data_ptr(), labels.data_ptr(), label_lens.data_ptr(),
                                                 act_lens.data_ptr(), A, N, costs.data_ptr(), frames.data_ptr() if emit else None,
                                                 ws.data_ptr(), opt, code)
                assert st == 0, st
            return fn

        for pen in PENALTIES:
            for emit in (False, True):
                ms["cabi%s_p%g" % ("_emit" if emit else "", pen)] = timed(step_cabi(pen, emit), a.steps, a.warmup)
        su = stage_us(step_cabi(PENALTIES[1], True))
        E = N * T * U * A * esz
        fwd = su["stats"] + su["lattice"] + su["coef"] + su["emit"]
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "A": A,
                          "logits_mb": round(E / 2 ** 20, 1), "ms": {k: round(v, 4) for k, v in ms.items()},
                          "cabi_p0.01_vs_p0": round(ms["cabi_p0.01"] / ms["cabi_p0"], 4),
                          "cabi_emit_vs_cabi": round(ms["cabi_emit_p0.01"] / ms["cabi_p0.01"], 4),
                          "module_vs_ar_open": round(ms["module_p0.01"] / ms["ar_open"], 4),
                          "module_vs_rnnt": round(ms["module_p0.01"] / ms["rnnt"], 4),
                          "stages_us": {k: round(v, 1) for k, v in su.items()},
                          "emit_share_of_forward": round(su["emit"] / fwd, 4) if fwd > 0 else None,
                          "cabi_hbm_frac": round(3 * E / (ms["cabi_p0.01"] * 1e-3) / 1e9 / HBM_GBS, 3)}), flush=True)
        del acts, grads, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
