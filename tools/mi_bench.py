#!/usr/bin/env python
"""Time the lattice primitive on px / py edge log-probabilities (libwarprnnt_mi.so, warprnnt_pytorch.mi) beside two yardsticks
that are not the code under test, at the lattice shapes of c3 (B=128, T=150, S=20), c4 (B=64, T=1500, S=300) and c2 (B=16,
T=150, S=40), fp32, regular type (and the one call of the modified type).
  module      : mutual_information_recursion(px, py).sum().backward(), px and py requiring grad (two phases)
  cabi        : compute_rnnt_mi, one call with device scores into preallocated gradients and workspace
  cabi_score  : the same call without gradients (pack and the forward sweep alone)
  cabi_mod    : the one call of the modified type on px[:, :, :T]
  torch       : (a) the same recursion in plain torch on the GPU -- px / py skewed once per step, then one torch.logaddexp per
                anti-diagonal and autograd for the occupations: what a user without the library writes today
  delay       : (b) the lattice + coefficient stages of the delay library at the same lattice shape, read from
                profiles/delay/delay_bench_run*.jsonl (median of the runs there; not run here)
Each line: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step (torch: --torch-steps steps, it takes hundreds of launches per step); per-stage device times of the
one call (torch.profiler, mean over a few steps, in a traced pass of its own behind the timed steps); pack + unpack over the
lattice stage they wrap; and module ms over torch ms.

Without --child this process never touches the GPU: it starts one child process per run and shape, each under a time limit
of its own (--limit seconds), three runs by default, stops at the first child that fails or runs out of time, and writes run
K's lines to profiles/mi/mi_bench_runK.jsonl.
Usage: python tools/mi_bench.py [--runs 3] [--steps K] [--warmup W] [--config c3 c4 c2] [--limit SECONDS]"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c3": (128, 150, 20), "c4": (64, 1500, 300), "c2": (16, 150, 40)}
STAGES = {"pack": ["mi_pack_kernel"],
          "lattice": ["ar_lattice_wave_kernel", "ar_lattice_block_kernel", "mono_lattice_wave_kernel",
                      "mono_lattice_block_kernel", "mi_score_kernel"],
          "unpack": ["mi_unpack_kernel"]}
FLOOR = -1.0e30         # the plain-torch recursion's "no edge": finite, so that autograd through logaddexp stays finite


def delay_yardstick(cfg):
    """Median over profiles/delay/delay_bench_run*.jsonl of the delay library's lattice + coef device time (us) at `cfg`."""
    vals = []
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "delay", "delay_bench_run*.jsonl"))):
        for line in open(path):
            rec = json.loads(line)
            if rec.get("config") == cfg:
                vals.append(rec["stages_us"]["lattice"] + rec["stages_us"]["coef"])
    return round(statistics.median(vals), 1) if vals else None


def child(a):
    for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
        sys.path.insert(0, p)
    import torch
    from warprnnt_pytorch import _side, mi

    def timed(fn, steps, warmup, window_s=1.0, grow=True):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        if grow:
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

    def torch_recursion(px, py):
        """score (B,) of the regular type over the full rectangle: skew, then one logaddexp per anti-diagonal."""
        B, S1, T = py.shape
        S, D = S1 - 1, S1 + T                                          # diagonals 0 .. S + T
        d = torch.arange(D - 1, device=px.device)[None, :]             # the edges from diagonal d to d + 1
        sx, sy = torch.arange(S, device=px.device)[:, None], torch.arange(S1, device=px.device)[:, None]
        tx, ty = d - sx, d - sy                                        # px[s, d - s], py[s, d - s]
        pxs = torch.where((tx >= 0) & (tx <= T), px.gather(2, tx.clamp(0, T).expand(B, S, D - 1)), px.new_tensor(FLOOR))
        pys = torch.where((ty >= 0) & (ty < T), py.gather(2, ty.clamp(0, T - 1).expand(B, S1, D - 1)), py.new_tensor(FLOOR))
        p = torch.full((B, S1), FLOOR, device=px.device, dtype=px.dtype)
        p[:, 0] = 0.0
        pad = torch.full((B, 1), FLOOR, device=px.device, dtype=px.dtype)
        for k in range(D - 1):
            p = torch.logaddexp(torch.cat((pad, p[:, :-1] + pxs[:, :, k]), 1), p + pys[:, :, k])
        return p[:, S]

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cfg = a.child
    B, T, S = CONFIGS[cfg]
    px = (torch.rand((B, S, T + 1), generator=gen, device=dev) * -3.0).requires_grad_(True)
    py = (torch.rand((B, S + 1, T), generator=gen, device=dev) * -3.0).requires_grad_(True)

    def step_module():
        px.grad = py.grad = None
        mi.mutual_information_recursion(px, py, validate=False).sum().backward()

    def step_torch():
        px.grad = py.grad = None
        torch_recursion(px, py).sum().backward()

    ms = {"module": timed(step_module, a.steps, a.warmup)}
    # the yardstick computes what the library computes, on this very tensor
    want = torch_recursion(px.detach().double(), py.detach().double())
    got = mi.mutual_information_recursion(px.detach(), py.detach(), validate=False)
    assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-5), (got, want)
    ms["torch"] = timed(step_torch, a.torch_steps, 1, grow=False)
    px.grad = py.grad = None
    xd, yd = px.detach(), py.detach()
    xm = xd[:, :, :T].contiguous()
    gx, gy, gm = torch.empty_like(xd), torch.empty_like(yd), torch.empty_like(xm)
    scores = torch.empty(B, device=dev)
    ws = torch.empty(mi.workspace_bytes(S, T, B, False, 0), dtype=torch.uint8, device=dev)
    opt = _side.options(dev, 0, T, S + 1)
    lib = mi.lib()

    def step_cabi(x, g, mod, grads=True):
        def fn():
            st = lib.compute_rnnt_mi(x.data_ptr(), yd.data_ptr(), None, S, T, B, mod, scores.data_ptr(),
                                     g.data_ptr() if grads else None, gy.data_ptr() if grads else None, ws.data_ptr(), opt, 0)
            assert st == 0, st
        return fn

    ms["cabi"] = timed(step_cabi(xd, gx, 0), a.steps, a.warmup)
    ms["cabi_score"] = timed(step_cabi(xd, gx, 0, False), a.steps, a.warmup)
    ms["cabi_mod"] = timed(step_cabi(xm, gm, 1), a.steps, a.warmup)
    su = stage_us(step_cabi(xd, gx, 0))
    sm = stage_us(step_cabi(xm, gm, 1))
    dl = delay_yardstick(cfg)
    print(json.dumps({"config": cfg, "dtype": "float32", "B": B, "T": T, "S": S,
                      "ms": {k: round(v, 4) for k, v in ms.items()},
                      "stages_us": {k: round(v, 1) for k, v in su.items()},
                      "stages_us_modified": {k: round(v, 1) for k, v in sm.items()},
                      "pack_unpack_over_lattice": round((su["pack"] + su["unpack"]) / su["lattice"], 4) if su["lattice"] else None,
                      "module_over_torch": round(ms["module"] / ms["torch"], 5),
                      "torch_over_module": round(ms["torch"] / ms["module"], 1),
                      "delay_lattice_coef_us": dl,
                      "stages_over_delay": round(sum(su.values()) / dl, 4) if dl else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--config", nargs="+", default=["c3", "c4", "c2"])
    ap.add_argument("--limit", type=float, default=150.0, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for run in range(1, a.runs + 1):
        path = os.path.join(a.out, "mi_bench_run%d.jsonl" % run)
        with open(path, "w") as f:
            for cfg in a.config:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--steps", str(a.steps), "--warmup",
                       str(a.warmup), "--torch-steps", str(a.torch_steps)]
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
