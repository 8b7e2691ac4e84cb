#!/usr/bin/env python
"""Best-path alignment against the score-only loss on the same inputs: compute_rnnt_align vs compute_rnnt_loss_async with
gradients == NULL (materialised c2 / c3 / c4 shapes of bench.py), and compute_rnnt_align_add vs compute_rnnt_loss_add_fwd_dt
without the backward preparation (additive joint, c3 shape).  Both calls run in the same workspace; the time per call is the
median of `steps` HIP-event intervals on the current stream after `warmup` calls.
Usage: python tools/align_bench.py [c2 c3 c4 add_c3] [--steps K] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "warp-transducer_amd"))
from warprnnt_pytorch import _lib  # noqa: E402

SHAPES = {"c2": (16, 150, 41, 28), "c3": (128, 150, 21, 5000), "c4": (64, 1500, 301, 50), "add_c3": (128, 150, 21, 5000)}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def run(name, steps, warmup):
    N, T, U, A = SHAPES[name]
    lib = _lib.lib()
    g = torch.Generator("cuda").manual_seed(0)
    labels = torch.randint(1, A, (N, U - 1), dtype=torch.int32, device="cuda", generator=g)
    xl = torch.full((N,), T, dtype=torch.int32, device="cuda")
    yl = torch.full((N,), U - 1, dtype=torch.int32, device="cuda")
    score = torch.empty(N, dtype=torch.float64, device="cuda")
    frames = torch.empty((N, U - 1), dtype=torch.int32, device="cuda")
    costs = torch.empty(N, dtype=torch.float32, device="cuda")
    opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream().cuda_stream, blank_label=0,
                           maxT=T, maxU=U, batch_first=True)
    if name.startswith("add_"):
        f = torch.randn((N, T, A), device="cuda", generator=g)
        p = torch.randn((N, U, A), device="cuda", generator=g)
        ws = torch.empty(_lib.workspace_bytes_add(T, U, N), dtype=torch.uint8, device="cuda")
        args = (f.data_ptr(), p.data_ptr(), labels.data_ptr(), yl.data_ptr(), xl.data_ptr(), A, N)

        def loss():
            _lib.check(lib.compute_rnnt_loss_add_fwd_dt(*args, costs.data_ptr(), ws.data_ptr(), opt, 0, 0, 0.0), "loss")

        def align():
            _lib.check(lib.compute_rnnt_align_add(*args, score.data_ptr(), frames.data_ptr(), ws.data_ptr(), opt, 0), "align")
    else:
        acts = torch.randn((N, T, U, A), device="cuda", generator=g)
        ws = torch.empty(_lib.workspace_bytes(T, U, N, True, 4), dtype=torch.uint8, device="cuda")

        def loss():
            _lib.check(lib.compute_rnnt_loss_async(acts.data_ptr(), None, labels.data_ptr(), yl.data_ptr(), xl.data_ptr(), A, N,
                                                   costs.data_ptr(), None, ws.data_ptr(), opt, 0), "loss")

        def align():
            _lib.check(lib.compute_rnnt_align(acts.data_ptr(), labels.data_ptr(), yl.data_ptr(), xl.data_ptr(), A, N,
                                              score.data_ptr(), frames.data_ptr(), ws.data_ptr(), opt, 0), "align")
    t_loss = timed(loss, steps, warmup)
    t_align = timed(align, steps, warmup)
    loss()
    align()
    torch.cuda.synchronize()
    ok = bool((score <= -costs.double() + 1e-3 * costs.double().abs().clamp(min=1)).all())
    return {"workload": name, "N": N, "T": T, "U": U, "A": A, "loss_score_only_ms": round(t_loss, 4),
            "align_ms": round(t_align, 4), "align_over_loss": round(t_align / t_loss, 3), "score_le_minus_cost": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["c2", "c3", "c4", "add_c3"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for w in a.workloads:
        print(json.dumps(run(w, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
