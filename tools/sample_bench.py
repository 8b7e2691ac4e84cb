#!/usr/bin/env python
"""Time the alignment sampler over px / py edge log-probabilities (libwarprnnt_sample.so, warprnnt_pytorch.sample) beside
yardsticks that are not the code under test, at the lattice shapes of c3 (B=128, T=150, S=20), c2 (B=16, T=150, S=40) and c4
(B=64, T=1500, S=300), regular and modified type, fp32 and bf16, K = 1, 16, 256 walks per sample.  Per shape, type and dtype:
  (a) sweep    : sample_fwd_kernel's device time beside expect_fwd_kernel's on the same edges (costs aliasing the weights) in
                 the same process: half the state, one transcendental chain fewer
  (b) walk     : sample_walk_kernel's device time per K, and per step of the longest walk (S + T regular, T modified)
  (c) call     : compute_rnnt_sample, wall ms per K, beside a plain-torch route on the device (fp32, regular type, at the shapes
                 of --torch-config): alpha by one logaddexp per anti-diagonal in fp64, the walk as one batched gather per step
  (d) scores   : path_scores(px, py, frames).sum().backward() per K beside the torch gather / cumsum route with autograd on the
                 same frames
Each wall time: mean ms per step over --steps (after --warmup) or as many more as fill a window of one second, one device
synchronisation per step; device times from torch.profiler, mean over a few steps, in a traced pass of its own.

Without --child this process never touches the GPU: it starts one child process per run and shape, each under a time limit
of its own (--limit seconds), three runs by default, stops at the first child that fails or runs out of time, and writes run
K's lines to <out>/sample_bench_runK.jsonl (profiles/sample by default).
Usage: python tools/sample_bench.py [--runs 3] [--steps K] [--warmup W] [--config c3 c2 c4] [--limit SECONDS] [--out DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"c3": (128, 150, 20), "c4": (64, 1500, 300), "c2": (16, 150, 40)}
KS = (1, 16, 256)
STAGES = {"fwd": ["sample_fwd_kernel"], "walk": ["sample_walk_kernel"], "weights": ["path_weights_kernel"],
          "edges": ["path_edges_kernel"], "expect_fwd": ["expect_fwd_kernel"]}


def child(a):
    for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
        sys.path.insert(0, p)
    import torch
    from warprnnt_pytorch import _side, expect, sample

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
                if any(n in e.name for n in names):            # (demangled or not)
                    out[s] += e.device_time / reps
        return {k: round(v, 1) for k, v in out.items() if v}

    def torch_sample(px, py, u):
        """The plain-torch route, regular type, full rectangle: alpha in fp64 by one logaddexp per anti-diagonal (skewed:
        A[b, d, s] = alpha[b, s, d - s]), then the K walks of every sample advanced together, one batched gather per operand
        and step.  -> frames (B, K, S), W (B, K), scores (B)."""
        B, S1, T = py.shape
        S, D = S1 - 1, S1 + T
        K = u.shape[1]
        dev = px.device
        x, y = px.double(), py.double()
        neg = float("-inf")
        d = torch.arange(D - 1, device=dev)[None, :]
        sx, sy = torch.arange(S, device=dev)[:, None], torch.arange(S1, device=dev)[:, None]
        tx, ty = d - sx, d - sy
        xs = torch.where((tx >= 0) & (tx <= T), x.gather(2, tx.clamp(0, T).expand(B, S, D - 1)), x.new_tensor(neg))
        ys = torch.where((ty >= 0) & (ty < T), y.gather(2, ty.clamp(0, T - 1).expand(B, S1, D - 1)), y.new_tensor(neg))
        A = torch.full((B, D, S1), neg, device=dev, dtype=torch.float64)
        A[:, 0, 0] = 0.0
        pad = torch.full((B, 1), neg, device=dev, dtype=torch.float64)
        for k in range(D - 1):
            p = A[:, k]
            A[:, k + 1] = torch.logaddexp(torch.cat((pad, p[:, :-1] + xs[:, :, k]), 1), p + ys[:, :, k])
        Af, xf, yf, uf = A.reshape(B, -1), x.reshape(B, -1), y.reshape(B, -1), u.double()
        s = torch.full((B, K), S, device=dev, dtype=torch.long)
        t = torch.full((B, K), T, device=dev, dtype=torch.long)
        W = torch.zeros((B, K), device=dev, dtype=torch.float64)
        frames = torch.full((B, K, max(S, 1)), -1, device=dev, dtype=torch.int32)
        for _ in range(S + T):
            sm, tm = (s - 1).clamp(min=0), (t - 1).clamp(min=0)
            cur = Af.gather(1, (s + t) * S1 + s)
            ax = Af.gather(1, (sm + t) * S1 + sm)
            wx = xf.gather(1, sm * (T + 1) + t) if S else cur
            wy = yf.gather(1, s * T + tm)
            uu = uf.gather(2, (s + t - 1).clamp(min=0)[:, :, None])[:, :, 0]
            live = (s > 0) | (t > 0)
            sym = live & (s > 0) & ((uu < torch.exp(ax + wx - cur)) | (t == 0))
            frames.scatter_(2, sm[:, :, None], torch.where(sym, t, frames.gather(2, sm[:, :, None])[:, :, 0].long()).int()[:, :, None])
            W = W + torch.where(sym, wx, torch.where(live, wy, torch.zeros_like(wy)))
            s, t = torch.where(sym, s - 1, s), torch.where(live & ~sym, t - 1, t)
        return frames[:, :, :S], W, A[:, D - 1, S]

    def torch_path_scores(px, py, frames):
        """W (B, K) of the regular type's full rectangle from frames (B, K, S): gathers of px and of the running sum of py."""
        B, S1, T = py.shape
        S = S1 - 1
        fr = frames.long()
        K = fr.shape[1]
        wx = px.double()[:, None].expand(B, K, S, T + 1).gather(3, fr[:, :, :, None])[:, :, :, 0].sum(2)
        c = torch.cat((torch.zeros((B, S1, 1), device=py.device, dtype=torch.float64), py.double().cumsum(2)), 2)
        lo = torch.cat((torch.zeros((B, K, 1), device=py.device, dtype=torch.long), fr), 2)
        hi = torch.cat((fr, torch.full((B, K, 1), T, device=py.device, dtype=torch.long)), 2)
        ce = c[:, None].expand(B, K, S1, T + 1)
        return wx + (ce.gather(3, hi[:, :, :, None]) - ce.gather(3, lo[:, :, :, None]))[:, :, :, 0].sum(2)

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    cfg = a.child
    B, T, S = CONFIGS[cfg]
    base_x = torch.rand((B, S, T + 1), generator=gen, device=dev) * -3.0
    base_y = torch.rand((B, S + 1, T), generator=gen, device=dev) * -3.0
    lib, elib = sample.lib(), expect.lib()
    opt = _side.options(dev, 0, T, S + 1)
    for dtype, code in ((torch.float32, 0), (torch.bfloat16, 2)):
        for mod in (0, 1):
            xd = (base_x[:, :, :T] if mod else base_x).to(dtype).contiguous()
            yd = base_y.to(dtype).contiguous()
            scores = torch.empty(B, dtype=torch.float64, device=dev)
            alpha = torch.empty((B, S + 1, T + 1), dtype=torch.float64, device=dev)
            ec = torch.empty(B, dtype=torch.float64, device=dev)
            nodes = torch.empty((B, S + 1, T + 1, 2), dtype=torch.float64, device=dev)

            def step_expect():
                st = elib.compute_rnnt_expect_fwd(xd.data_ptr(), yd.data_ptr(), xd.data_ptr(), yd.data_ptr(), None, S, T, B, mod,
                                                  scores.data_ptr(), ec.data_ptr(), nodes.data_ptr(), opt, code)
                assert st == 0, st

            line = {"config": cfg, "dtype": str(dtype).split(".")[-1], "type": "modified" if mod else "regular", "B": B, "T": T,
                    "S": S, "steps": T if mod else S + T, "expect_fwd_ms": round(timed(step_expect, a.steps, a.warmup), 4),
                    "expect_fwd_us": stage_us(step_expect).get("expect_fwd"), "K": {}}
            for K in KS:
                u = torch.rand((B, K, S + T), generator=gen, device=dev)
                frames = torch.empty((B, K, S), dtype=torch.int32, device=dev)
                weights = torch.empty((B, K), dtype=torch.float64, device=dev)

                def step_sample():
                    st = lib.compute_rnnt_sample(xd.data_ptr(), yd.data_ptr(), None, u.data_ptr(), S, T, B, K, mod, scores.data_ptr(),
                                                 alpha.data_ptr(), frames.data_ptr(), weights.data_ptr(), opt, code)
                    assert st == 0, st

                xa, ya = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)

                def step_scores():
                    xa.grad = ya.grad = None
                    sample.path_scores(xa, ya, frames, validate=False).sum().backward()

                r = {"call_ms": round(timed(step_sample, a.steps, a.warmup), 4)}
                su = stage_us(step_sample)
                r["fwd_us"], r["walk_us"] = su.get("fwd"), su.get("walk")
                r["walk_us_per_step"] = round(su.get("walk", 0.0) / line["steps"], 4)
                r["scores_ms"] = round(timed(step_scores, a.steps, a.warmup), 4)
                sv = stage_us(step_scores)
                r["weights_us"], r["edges_us"] = sv.get("weights"), sv.get("edges")
                if cfg in a.torch_config and not mod and code == 0:
                    # the yardstick computes what the library computes, on these very tensors and uniforms
                    tf, tw, ts = torch_sample(xd, yd, u)
                    step_sample()
                    torch.cuda.synchronize()
                    same = (tf == frames).all(2)
                    assert same.float().mean() > 0.999 and torch.allclose(ts, scores, rtol=1e-9), same.float().mean()
                    assert torch.allclose(tw[same], weights[same], rtol=1e-9, atol=1e-9)
                    r["torch_call_ms"] = round(timed(lambda: torch_sample(xd, yd, u), a.torch_steps, 1, grow=False), 3)
                    want = torch_path_scores(xd, yd, frames)
                    assert torch.allclose(want, weights, rtol=1e-9, atol=1e-9)

                    def step_torch_scores():
                        xa.grad = ya.grad = None
                        torch_path_scores(xa, ya, frames).sum().backward()

                    r["torch_scores_ms"] = round(timed(step_torch_scores, a.torch_steps, 1, grow=False), 3)
                    r["torch_over_call"] = round(r["torch_call_ms"] / r["call_ms"], 1)
                    r["torch_over_scores"] = round(r["torch_scores_ms"] / r["scores_ms"], 1)
                line["K"][str(K)] = r
            k1 = line["K"]["1"]
            line["fwd_over_expect_fwd"] = round(k1["fwd_us"] / line["expect_fwd_us"], 4) if line["expect_fwd_us"] and k1["fwd_us"] else None
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--torch-config", nargs="*", default=["c3", "c2"], help="shapes at which the plain-torch route is run")
    ap.add_argument("--config", nargs="+", default=["c3", "c2", "c4"])
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    for run in range(1, a.runs + 1):
        path = os.path.join(a.out, "sample_bench_run%d.jsonl" % run)
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
                for line in r.stdout.strip().splitlines():
                    if line.startswith("{"):
                        f.write(line + "\n")
                        print("run %d %s" % (run, line), flush=True)
                f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
