#!/usr/bin/env python
"""Time the expected path cost over px / py edge log-probabilities (libwarprnnt_expect.so, warprnnt_pytorch.expect) beside
yardsticks that are not the code under test, at the lattice shapes of c3 (B=128, T=150, S=20), c4 (B=64, T=1500, S=300) and
c2 (B=16, T=150, S=40), fp32, regular type (and the one call of the modified type).
  module       : expected_cost(px, py, cx, cy).sum().backward(), all four requiring grad (the forward launch, then the backward)
  entropy      : alignment_entropy(px, py).sum().backward()
  cabi         : compute_rnnt_expect, one call with device scalars and all four gradients into preallocated outputs
  cabi_nocost  : the same call without cx_grad / cy_grad
  cabi_fwd     : the same call without gradients (the forward launch alone)
  cabi_mod     : the one call of the modified type on px[:, :, :T]
  mi           : compute_rnnt_mi of this tree on the same px / py with gradients, and mi_score: score only -- the log-sum
                 semiring over the same lattice (first order: it cannot give the weight gradient of an expectation)
  torch        : plain torch on the GPU, at the shapes of --torch-config: log Z(px + lam cx, py + lam cy) by one
                 log-add per anti-diagonal, E[C] = d log Z / d lam at lam = 0 with create_graph=True, then backward
                 through that gradient (double backward): what a user without the library writes today
Each line: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step (torch: --torch-steps steps); per-stage device times of the one call (torch.profiler, mean over a
few steps, in a traced pass of its own behind the timed steps) beside mi's.

Without --child this process never touches the GPU: it starts one child process per run and shape, each under a time limit
of its own (--limit seconds), three runs by default, stops at the first child that fails or runs out of time, and writes run
K's lines to profiles/expect/expect_bench_runK.jsonl.
Usage: python tools/expect_bench.py [--runs 3] [--steps K] [--warmup W] [--config c3 c4 c2] [--limit SECONDS]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c3": (128, 150, 20), "c4": (64, 1500, 300), "c2": (16, 150, 40)}
STAGES = {"fwd": ["expect_fwd_kernel"], "bwd": ["expect_bwd_kernel"]}
MI_STAGES = {"pack": ["mi_pack_kernel"],
             "lattice": ["ar_lattice_wave_kernel", "ar_lattice_block_kernel", "mono_lattice_wave_kernel",
                         "mono_lattice_block_kernel", "mi_score_kernel"],
             "unpack": ["mi_unpack_kernel"]}


def child(a):
    for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
        sys.path.insert(0, p)
    import torch
    from warprnnt_pytorch import _side, expect, mi

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

    def torch_logz(px, py):
        """log Z (B,) of the regular type over the full rectangle: skew, then one log-add per anti-diagonal.  The log-add is
        written out around a detached maximum: the second derivative of torch.logaddexp is inf / inf = NaN wherever its
        arguments are more than 709 apart, which the floor of the skewed layout always is."""
        B, S1, T = py.shape
        S, D = S1 - 1, S1 + T
        d = torch.arange(D - 1, device=px.device)[None, :]
        sx, sy = torch.arange(S, device=px.device)[:, None], torch.arange(S1, device=px.device)[:, None]
        tx, ty = d - sx, d - sy
        low = -1e30                                            # (a finite floor: -inf - -inf is NaN)

        def lae(u, v):
            m = torch.maximum(u, v).detach()
            return m + torch.log(torch.exp(u - m) + torch.exp(v - m))

        pxs = torch.where((tx >= 0) & (tx <= T), px.gather(2, tx.clamp(0, T).expand(B, S, D - 1)), px.new_tensor(low))
        pys = torch.where((ty >= 0) & (ty < T), py.gather(2, ty.clamp(0, T - 1).expand(B, S1, D - 1)), py.new_tensor(low))
        p = torch.full((B, S1), low, device=px.device, dtype=px.dtype)
        p[:, 0] = 0.0
        pad = torch.full((B, 1), low, device=px.device, dtype=px.dtype)
        for k in range(D - 1):
            p = lae(torch.cat((pad, p[:, :-1] + pxs[:, :, k]), 1), p + pys[:, :, k])
        return p[:, S]

    def torch_expected(px, py, cx, cy):
        """E[C] (B,) as d log Z(w + lam c) / d lam at lam = 0, differentiable once more."""
        lam = torch.zeros((px.shape[0], 1, 1), device=px.device, dtype=px.dtype, requires_grad=True)
        logz = torch_logz(px + lam * cx, py + lam * cy)
        return torch.autograd.grad(logz.sum(), lam, create_graph=True)[0].reshape(-1)

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cfg = a.child
    B, T, S = CONFIGS[cfg]
    px = (torch.rand((B, S, T + 1), generator=gen, device=dev) * -3.0).requires_grad_(True)
    py = (torch.rand((B, S + 1, T), generator=gen, device=dev) * -3.0).requires_grad_(True)
    cx = torch.arange(T + 1.0, device=dev).expand(B, S, T + 1).contiguous().requires_grad_(True)     # the latency recipe
    cy = torch.zeros((B, S + 1, T), device=dev).requires_grad_(True)
    leaves = (px, py, cx, cy)

    def step_module():
        for t in leaves:
            t.grad = None
        expect.expected_cost(px, py, cx, cy, validate=False).sum().backward()

    def step_entropy():
        px.grad = py.grad = None
        expect.alignment_entropy(px, py, validate=False).sum().backward()

    ms = {"module": timed(step_module, a.steps, a.warmup), "entropy": timed(step_entropy, a.steps, a.warmup)}
    for t in leaves:
        t.grad = None
    xd, yd, cxd, cyd = (t.detach() for t in leaves)
    if cfg in a.torch_config:
        # the yardstick computes what the library computes, on these very tensors (fp64 both)
        x64, y64 = xd.double().requires_grad_(True), yd.double().requires_grad_(True)
        want = torch_expected(x64, y64, cxd.double(), cyd.double())
        want.sum().backward()
        xl, yl = xd.double().requires_grad_(True), yd.double().requires_grad_(True)
        got = expect.expected_cost(xl, yl, cxd.double(), cyd.double(), validate=False)
        got.sum().backward()
        assert torch.allclose(got, want, rtol=1e-9, atol=1e-9), (got, want)
        assert torch.allclose(xl.grad, x64.grad, rtol=1e-7, atol=1e-9) and torch.allclose(yl.grad, y64.grad, rtol=1e-7, atol=1e-9)
        del x64, y64, xl, yl, want, got

        def step_torch():
            px.grad = py.grad = None
            torch_expected(px, py, cxd, cyd).sum().backward()

        ms["torch"] = timed(step_torch, a.torch_steps, 1, grow=False)
        px.grad = py.grad = None
    xm, cxm = xd[:, :, :T].contiguous(), cxd[:, :, :T].contiguous()
    gx, gy, hx, hy = torch.empty_like(xd), torch.empty_like(yd), torch.empty_like(xd), torch.empty_like(yd)
    gm, hm = torch.empty_like(xm), torch.empty_like(xm)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    ec = torch.empty(B, dtype=torch.float64, device=dev)
    nodes = torch.empty((B, S + 1, T + 1, 2), dtype=torch.float64, device=dev)
    opt = _side.options(dev, 0, T, S + 1)
    lib = expect.lib()

    def step_cabi(x, c, g, h, mod, grads=True, costs=True):
        def fn():
            st = lib.compute_rnnt_expect(x.data_ptr(), yd.data_ptr(), c.data_ptr(), cyd.data_ptr(), None, S, T, B, mod,
                                         scores.data_ptr(), ec.data_ptr(), nodes.data_ptr(), g.data_ptr() if grads else None,
                                         gy.data_ptr() if grads else None, h.data_ptr() if grads and costs else None,
                                         hy.data_ptr() if grads and costs else None, opt, 0)
            assert st == 0, st
        return fn

    ms["cabi"] = timed(step_cabi(xd, cxd, gx, hx, 0), a.steps, a.warmup)
    ms["cabi_nocost"] = timed(step_cabi(xd, cxd, gx, hx, 0, costs=False), a.steps, a.warmup)
    ms["cabi_fwd"] = timed(step_cabi(xd, cxd, gx, hx, 0, grads=False), a.steps, a.warmup)
    ms["cabi_mod"] = timed(step_cabi(xm, cxm, gm, hm, 1), a.steps, a.warmup)
    su = stage_us(step_cabi(xd, cxd, gx, hx, 0), STAGES)
    sm = stage_us(step_cabi(xm, cxm, gm, hm, 1), STAGES)

    # yardstick: the log-sum lattice of this tree on the same edges
    mscores = torch.empty(B, device=dev)
    ws = torch.empty(mi.workspace_bytes(S, T, B, False, 0), dtype=torch.uint8, device=dev)
    mlib = mi.lib()

    def step_mi(grads):
        def fn():
            st = mlib.compute_rnnt_mi(xd.data_ptr(), yd.data_ptr(), None, S, T, B, 0, mscores.data_ptr(),
                                      gx.data_ptr() if grads else None, gy.data_ptr() if grads else None, ws.data_ptr(), opt, 0)
            assert st == 0, st
        return fn

    ms["mi"] = timed(step_mi(True), a.steps, a.warmup)
    ms["mi_score"] = timed(step_mi(False), a.steps, a.warmup)
    mu = stage_us(step_mi(True), MI_STAGES)

    steps = T + S + 1
    print(json.dumps({"config": cfg, "dtype": "float32", "B": B, "T": T, "S": S,
                      "ms": {k: round(v, 4) for k, v in ms.items()},
                      "stages_us": su, "stages_us_modified": sm, "mi_stages_us": mu,
                      "cabi_over_mi": round(ms["cabi"] / ms["mi"], 4),
                      "device_over_mi_device": round(sum(su.values()) / sum(mu.values()), 4) if sum(mu.values()) else None,
                      "fwd_us_per_step": round(su["fwd"] / steps, 3), "bwd_us_per_step": round(su["bwd"] / steps, 3),
                      "torch_over_module": round(ms["torch"] / ms["module"], 1) if "torch" in ms else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--torch-config", nargs="*", default=["c3", "c2"], help="shapes at which the plain-torch route is run")
    ap.add_argument("--config", nargs="+", default=["c3", "c4", "c2"])
    ap.add_argument("--limit", type=float, default=150.0, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expect"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for run in range(1, a.runs + 1):
        path = os.path.join(a.out, "expect_bench_run%d.jsonl" % run)
        with open(path, "w") as f:
            for cfg in a.config:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--steps", str(a.steps), "--warmup",
                       str(a.warmup), "--torch-steps", str(a.torch_steps), "--torch-config"] + list(a.torch_config)
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
