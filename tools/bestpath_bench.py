#!/usr/bin/env python
"""Time the best path over px / py edge log-probabilities (libwarprnnt_bestpath.so, warprnnt_pytorch.bestpath) beside
yardsticks that are not the code under test, at the lattice shapes of c3 (B=128, T=150, S=20), c4 (B=64, T=1500, S=300) and
c2 (B=16, T=150, S=40), fp32, regular type (and the one call of the modified type).
  module       : best_path(px, py)[0].sum().backward(), px and py requiring grad (the sweep launch, then the edges entry)
  cabi         : compute_rnnt_bestpath, one call with device scores and both indicators into preallocated outputs
  cabi_noedges : the same call without px_path / py_path (the sweep launch alone)
  cabi_mod     : the one call of the modified type on px[:, :, :T]
  mi           : compute_rnnt_mi of this tree on the same px / py with gradients, and mi_score: score only -- the log-sum
                 semiring over the same lattice, which the feature leaves untouched
  align        : rnnt_align on logits (B, T, S + 1, --classes) of the same lattice: the whole call, and the device time of its
                 lattice and traceback kernels alone (the statistics stage reads the logits, which best_path never sees)
  torch        : a plain-torch max-plus sweep on the GPU, px / py skewed once per step, one torch.maximum per anti-diagonal,
                 scores only: what a user without the library writes today
Each line: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step (torch: --torch-steps steps); per-stage device times of the one call (torch.profiler, mean over a
few steps, in a traced pass of its own behind the timed steps) beside mi's and rnnt_align's.

Without --child this process never touches the GPU: it starts one child process per run and shape, each under a time limit
of its own (--limit seconds), three runs by default, stops at the first child that fails or runs out of time, and writes run
K's lines to profiles/bestpath/bestpath_bench_runK.jsonl.
Usage: python tools/bestpath_bench.py [--runs 3] [--steps K] [--warmup W] [--config c3 c4 c2] [--limit SECONDS]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c3": (128, 150, 20), "c4": (64, 1500, 300), "c2": (16, 150, 40)}
STAGES = {"sweep": ["bestpath_sweep_kernel"], "edges": ["bestpath_edges_kernel"]}
MI_STAGES = {"pack": ["mi_pack_kernel"],
             "lattice": ["ar_lattice_wave_kernel", "ar_lattice_block_kernel", "mono_lattice_wave_kernel",
                         "mono_lattice_block_kernel", "mi_score_kernel"],
             "unpack": ["mi_unpack_kernel"]}
ALIGN_STAGES = {"lattice": ["align_lattice_kernel"], "traceback": ["align_traceback_kernel"]}
FLOOR = float("-inf")


def child(a):
    for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
        sys.path.insert(0, p)
    import torch
    from warprnnt_pytorch import _side, bestpath, mi, rnnt_align

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

    def stage_us(fn, stages, reps=5):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {s: 0.0 for s in stages}
        for e in prof.events():
            if e.device_type != DeviceType.CUDA:
                continue
            for s, names in stages.items():
                if any(n in e.name for n in names):            # (demangled or not)
                    out[s] += e.device_time / reps
        return {k: round(v, 1) for k, v in out.items()}

    def torch_maxplus(px, py):
        """score (B,) of the regular type over the full rectangle: skew, then one torch.maximum per anti-diagonal."""
        B, S1, T = py.shape
        S, D = S1 - 1, S1 + T
        d = torch.arange(D - 1, device=px.device)[None, :]
        sx, sy = torch.arange(S, device=px.device)[:, None], torch.arange(S1, device=px.device)[:, None]
        tx, ty = d - sx, d - sy
        pxs = torch.where((tx >= 0) & (tx <= T), px.gather(2, tx.clamp(0, T).expand(B, S, D - 1)), px.new_tensor(FLOOR))
        pys = torch.where((ty >= 0) & (ty < T), py.gather(2, ty.clamp(0, T - 1).expand(B, S1, D - 1)), py.new_tensor(FLOOR))
        p = torch.full((B, S1), FLOOR, device=px.device, dtype=px.dtype)
        p[:, 0] = 0.0
        pad = torch.full((B, 1), FLOOR, device=px.device, dtype=px.dtype)
        for k in range(D - 1):
            p = torch.maximum(torch.cat((pad, p[:, :-1] + pxs[:, :, k]), 1), p + pys[:, :, k])
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
        bestpath.best_path(px, py, validate=False)[0].sum().backward()

    ms = {"module": timed(step_module, a.steps, a.warmup)}
    px.grad = py.grad = None
    xd, yd = px.detach(), py.detach()
    # the yardstick computes what the library computes, on this very tensor (fp64 both: the same additions)
    want = torch_maxplus(xd.double(), yd.double())
    got = bestpath.best_path(xd.double(), yd.double(), validate=False)[0]
    assert torch.equal(got, want), (got, want)
    ms["torch"] = timed(lambda: torch_maxplus(xd, yd), a.torch_steps, 1, grow=False)
    xm = xd[:, :, :T].contiguous()
    ex, ey, em = torch.empty_like(xd), torch.empty_like(yd), torch.empty_like(xm)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    frames = torch.empty((B, S), dtype=torch.int32, device=dev)
    back = torch.empty((B, S + 1, bestpath.back_words(T)), dtype=torch.int64, device=dev)
    opt = _side.options(dev, 0, T, S + 1)
    lib = bestpath.lib()

    def step_cabi(x, g, mod, edges=True):
        def fn():
            st = lib.compute_rnnt_bestpath(x.data_ptr(), yd.data_ptr(), None, S, T, B, mod, scores.data_ptr(), frames.data_ptr(),
                                           back.data_ptr(), g.data_ptr() if edges else None, ey.data_ptr() if edges else None,
                                           opt, 0)
            assert st == 0, st
        return fn

    ms["cabi"] = timed(step_cabi(xd, ex, 0), a.steps, a.warmup)
    ms["cabi_noedges"] = timed(step_cabi(xd, ex, 0, False), a.steps, a.warmup)
    ms["cabi_mod"] = timed(step_cabi(xm, em, 1), a.steps, a.warmup)
    su = stage_us(step_cabi(xd, ex, 0), STAGES)
    sm = stage_us(step_cabi(xm, em, 1), STAGES)

    # yardstick: the log-sum lattice of this tree on the same edges
    mscores = torch.empty(B, device=dev)
    ws = torch.empty(mi.workspace_bytes(S, T, B, False, 0), dtype=torch.uint8, device=dev)
    mlib = mi.lib()

    def step_mi(grads):
        def fn():
            st = mlib.compute_rnnt_mi(xd.data_ptr(), yd.data_ptr(), None, S, T, B, 0, mscores.data_ptr(),
                                      ex.data_ptr() if grads else None, ey.data_ptr() if grads else None, ws.data_ptr(), opt, 0)
            assert st == 0, st
        return fn

    ms["mi"] = timed(step_mi(True), a.steps, a.warmup)
    ms["mi_score"] = timed(step_mi(False), a.steps, a.warmup)
    mu = stage_us(step_mi(True), MI_STAGES)
    mu_score = stage_us(step_mi(False), MI_STAGES)
    del ws

    # yardstick: rnnt_align on logits of the same lattice
    logits = torch.randn((B, T, S + 1, a.classes), generator=gen, device=dev)
    labels = torch.randint(1, a.classes, (B, S), generator=gen, device=dev, dtype=torch.int32)
    xl = torch.full((B,), T, dtype=torch.int32, device=dev)
    yl = torch.full((B,), S, dtype=torch.int32, device=dev)
    step_align = lambda: rnnt_align(logits, labels, xl, yl)                                  # noqa: E731
    ms["align"] = timed(step_align, a.steps, a.warmup)
    au = stage_us(step_align, ALIGN_STAGES)

    print(json.dumps({"config": cfg, "dtype": "float32", "B": B, "T": T, "S": S, "classes": a.classes,
                      "ms": {k: round(v, 4) for k, v in ms.items()},
                      "stages_us": su, "stages_us_modified": sm, "mi_stages_us": mu, "mi_score_stages_us": mu_score,
                      "align_stages_us": au,
                      "cabi_over_mi": round(ms["cabi"] / ms["mi"], 4),
                      "sweep_over_mi_forward_lattice": round(su["sweep"] / mu_score["lattice"], 4) if mu_score["lattice"] else None,
                      "sweep_over_align_lattice_traceback": round(su["sweep"] / sum(au.values()), 4) if sum(au.values()) else None,
                      "torch_over_cabi_noedges": round(ms["torch"] / ms["cabi_noedges"], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--classes", type=int, default=8, help="classes of the logits rnnt_align is given")
    ap.add_argument("--config", nargs="+", default=["c3", "c4", "c2"])
    ap.add_argument("--limit", type=float, default=150.0, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bestpath"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for run in range(1, a.runs + 1):
        path = os.path.join(a.out, "bestpath_bench_run%d.jsonl" % run)
        with open(path, "w") as f:
            for cfg in a.config:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--steps", str(a.steps), "--warmup",
                       str(a.warmup), "--torch-steps", str(a.torch_steps), "--classes", str(a.classes)]
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
