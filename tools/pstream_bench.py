#!/usr/bin/env python
"""Time the pruned loss with lattice type and delay penalty (libwarprnnt_pstream.so) beside the routes the tree had before
it, on the same (N, T, S, A) tensor in the same process.
  cabi_t{0,1}_p{0,0.01}    : compute_rnnt_loss_pstream, one call with device costs into preallocated gradients and workspace
  module_t{0,1}_p{0,0.01}  : PrunedStreamingRNNTLoss(blank=A - 1, reduction='mean', validate=False), forward + backward
  pruned_cabi, pruned_module : compute_rnnt_loss_pruned / RNNTLossPruned on the same tensor and windows -- the yardstick,
                             timed before AND after this library's rows (both values and their mean are reported)
  torch_mi                 : the route without this library: log_softmax, gathers of the blank and label columns, a scatter
                             into px (N, L, T + 1) / py (N, L + 1, T) with -inf outside the windows, then
                             warprnnt_pytorch.mi.mutual_information_recursion, forward + backward; its peak device memory
                             beside the module's
Shapes: c3 (N=128, T=150, L=20, A=5000) fp32 and bf16 at S = 4 and 8; c5 (N=128, T=200, L=40, A=1024, bf16) at S = 5; c4
(N=64, T=1500, L=300, A=50, fp32) at S = 5.  Windows: S states around the diagonal u = t L / T, a path for both types.  Each
line: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step, every shape warmed up; per-stage device times of this library's call (type 0 and type 1 at 0.01) and
of the pruned library's (torch.profiler, mean over a few steps, in a TRACED pass of its own behind the timed steps); and the
fraction of the 8 TB/s HBM roofline the two streaming kernels reach on their algorithmic bytes: the rows read once for the
statistics kernel, every row written and the read rows read once for the gradient stream -- with the same figures for the
pruned library's kernels.  Run it in three processes and take medians.
Usage: python tools/pstream_bench.py [--steps K] [--warmup W] [--config c3_f32_s4 ...]"""
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
CONFIGS = {"c3_f32_s4": (128, 150, 20, 5000, torch.float32, 4), "c3_f32_s8": (128, 150, 20, 5000, torch.float32, 8),
           "c3_bf16_s4": (128, 150, 20, 5000, torch.bfloat16, 4), "c3_bf16_s8": (128, 150, 20, 5000, torch.bfloat16, 8),
           "c5_bf16_s5": (128, 200, 40, 1024, torch.bfloat16, 5), "c4_f32_s5": (64, 1500, 300, 50, torch.float32, 5)}
STAGES = {"prep": ["pstream_prep_kernel", "pruned_prep_kernel"], "stats": ["pstream_stats_kernel", "pruned_stats_kernel"],
          "lattice": ["ar_lattice_wave_kernel", "ar_lattice_block_kernel", "mono_lattice_wave_kernel", "mono_lattice_block_kernel",
                      "lattice_kernel", "lattice_lin_kernel"],
          "close": ["pstream_close_kernel", "pruned_fix_kernel"], "coef": ["pstream_coef_kernel", "coef_cell_kernel", "coef_kernel"],
          "grad": ["mblank_grad_kernel", "mblank_grad_elem_kernel", "pruned_grad_kernel", "pruned_grad_elem_kernel"]}
ROWS = ((0, 0.0), (0, 0.01), (1, 0.0), (1, 0.01))


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
            if any(("::" + n + "<") in e.name for n in names):
                out[s] += e.device_time / reps
    return out


def diagonal_windows(N, T, L, S, dev):
    """(N, T) int32: s_t = clamp(round(t L / T) - S // 2, 0, max(0, L + 1 - S)); steps of at most one state per frame."""
    t = torch.arange(T, device=dev, dtype=torch.float64)
    s = (torch.round(t * L / T) - S // 2).clamp(0, max(0, L + 1 - S)).to(torch.int32)
    return s.unsqueeze(0).expand(N, T).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS))
    a = ap.parse_args()
    from warprnnt_pytorch import _side, pruned, pstream
    from warprnnt_pytorch.mi import mutual_information_recursion
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for cfg in a.config:
        N, T, L, A, dt, S = CONFIGS[cfg]
        U, blank = L + 1, A - 1
        esz = torch.finfo(dt).bits // 8
        code = _side.DT[dt]
        labels = torch.randint(0, A - 1, (N, L), generator=gen, device=dev, dtype=torch.int32)
        act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
        label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
        ranges = diagonal_windows(N, T, L, S, dev)
        acts = torch.rand((N, T, S, A), generator=gen, device=dev).to(dt).requires_grad_(True)
        # rows of the tensor inside the lattice, and of those inside the modified type's band
        u = ranges.long().unsqueeze(-1) + torch.arange(S, device=dev)
        tt = torch.arange(T, device=dev).view(1, T, 1)
        inl = u <= L
        band = inl & (u <= tt) & (L - u <= T - tt)
        rows_all, rows_read = N * T * S, {0: int(inl.sum()), 1: int(band.sum())}

        def step_module(m):
            def fn():
                acts.grad = None
                m(acts, labels, act_lens, label_lens, ranges).backward()
            return fn

        # the torch route to the px / py primitive (the regular type; its penalty would be one more add on px)
        idx = u.clamp(max=L)
        lab_at = torch.gather(labels.long().unsqueeze(1).expand(N, T, L), 2, u.clamp(max=L - 1))

        def step_torch():
            acts.grad = None
            lp = torch.log_softmax(acts.float(), -1)
            ninf = torch.full((N, T, U), float("-inf"), device=dev)
            pyv = torch.where(inl, lp[..., blank], ninf[..., :S])
            pxv = torch.where(u < L, torch.gather(lp, 3, lab_at.unsqueeze(-1)).squeeze(-1), ninf[..., :S])
            py = ninf.scatter(2, idx, pyv).transpose(1, 2).contiguous()
            px = ninf.scatter(2, idx, pxv)[..., :L].transpose(1, 2)
            px = torch.cat((px, ninf[:, :1, :L].transpose(1, 2)), 2).contiguous()
            (-mutual_information_recursion(px, py, validate=False)).mean().backward()

        pruned_module = pruned.RNNTLossPruned(blank=blank, reduction="mean", validate=False)
        acts.grad = None
        cdt = torch.float64 if dt == torch.float64 else torch.float32
        grads = torch.empty_like(acts)
        costs = torch.empty(N, dtype=cdt, device=dev)
        ws = torch.empty(max(pstream.workspace_bytes(T, U, S, N, code), pruned.workspace_bytes(T, U, N, code)), dtype=torch.uint8,
                         device=dev)
        opt = _side.options(dev, blank, T, U)
        lens = (labels.data_ptr(), label_lens.data_ptr(), act_lens.data_ptr(), A, N)

        def step_cabi(typ, pen):
            def fn():
                st = pstream.lib().compute_rnnt_loss_pstream(acts.data_ptr(), grads.data_ptr(), ranges.data_ptr(), S, typ, pen,
                                                             *lens, costs.data_ptr(), ws.data_ptr(), opt, code)
                assert st == 0, st
            return fn

        def step_pruned_cabi():
            st = pruned.lib().compute_rnnt_loss_pruned(acts.data_ptr(), grads.data_ptr(), ranges.data_ptr(), S, *lens,
                                                       costs.data_ptr(), ws.data_ptr(), opt, code)
            assert st == 0, st

        ms = {}
        ms["pruned_cabi_before"] = timed(step_pruned_cabi, a.steps, a.warmup)
        for typ, pen in ROWS:
            ms["cabi_t%d_p%g" % (typ, pen)] = timed(step_cabi(typ, pen), a.steps, a.warmup)
        ms["pruned_cabi_after"] = timed(step_pruned_cabi, a.steps, a.warmup)
        ms["pruned_cabi"] = 0.5 * (ms["pruned_cabi_before"] + ms["pruned_cabi_after"])
        ms["pruned_module_before"] = timed(step_module(pruned_module), a.steps, a.warmup)
        peak = {}
        for typ, pen in ROWS:
            m = pstream.PrunedStreamingRNNTLoss(blank, ("regular", "modified")[typ], pen, "mean", validate=False)
            torch.cuda.reset_peak_memory_stats(dev)
            ms["module_t%d_p%g" % (typ, pen)] = timed(step_module(m), a.steps, a.warmup)
            peak["module_t%d" % typ] = torch.cuda.max_memory_allocated(dev)
        ms["pruned_module_after"] = timed(step_module(pruned_module), a.steps, a.warmup)
        ms["pruned_module"] = 0.5 * (ms["pruned_module_before"] + ms["pruned_module_after"])
        torch.cuda.reset_peak_memory_stats(dev)
        ms["torch_mi"] = timed(step_torch, a.steps, a.warmup)
        peak["torch_mi"] = torch.cuda.max_memory_allocated(dev)
        acts.grad = None
        su = {"t0": stage_us(step_cabi(0, 0.01)), "t1": stage_us(step_cabi(1, 0.01)), "pruned": stage_us(step_pruned_cabi)}
        row_bytes = A * esz

        def frac(nbytes, us):
            return round(nbytes / (us * 1e-6) / 1e9 / HBM_GBS, 3) if us > 0 else None

        roof = {}
        for key, typ in (("t0", 0), ("t1", 1), ("pruned", 0)):
            roof[key] = {"stats": frac(rows_read[typ] * row_bytes, su[key]["stats"]),
                         "grad": frac((rows_all + rows_read[typ]) * row_bytes, su[key]["grad"])}
        E = rows_all * row_bytes
        print(json.dumps({"config": cfg, "dtype": str(dt).split(".")[-1], "N": N, "T": T, "U": U, "S": S, "A": A,
                          "logits_mb": round(E / 2 ** 20, 1), "rows": rows_all, "rows_read": rows_read,
                          "ms": {k: round(v, 4) for k, v in ms.items()},
                          "cabi_t0_p0_vs_pruned": round(ms["cabi_t0_p0"] / ms["pruned_cabi"], 4),
                          "pruned_cabi_spread": round(abs(ms["pruned_cabi_before"] - ms["pruned_cabi_after"]) / ms["pruned_cabi"], 4),
                          "cabi_t0_p0.01_vs_p0": round(ms["cabi_t0_p0.01"] / ms["cabi_t0_p0"], 4),
                          "cabi_t1_p0.01_vs_p0": round(ms["cabi_t1_p0.01"] / ms["cabi_t1_p0"], 4),
                          "module_t0_p0_vs_pruned": round(ms["module_t0_p0"] / ms["pruned_module"], 4),
                          "torch_mi_vs_module_t0": round(ms["torch_mi"] / ms["module_t0_p0"], 4),
                          "peak_mb": {k: round(v / 2 ** 20, 1) for k, v in peak.items()},
                          "stages_us": {k: {s: round(v, 1) for s, v in d.items()} for k, d in su.items()},
                          "hbm_frac": roof}), flush=True)
        del acts, grads, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
