"""bench.py's launcher contract without a GPU: it must fail loudly (exit code 2, nothing on stdout) instead of
falling back to a CPU path or to fewer GPUs than requested.  (The GPU-side cases live in
tests/test_gpu_sharded_rccl.py.)"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only contract")
@pytest.mark.parametrize("gpus", ["1", "2", "8"])
def test_bench_needs_a_gpu(gpus):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", gpus], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 2 and not out.stdout.strip()
    assert "MI355X" in out.stderr


EXPECTED_OTHER = {"c2", "c4", "c5_per_gpu", "c5_full_1024_on_one_gpu", "add_c3_f32", "add_c3_bf16", "add_c4_f32",
                  "rnntloss_c3", "rnntloss_c5", "rnntloss_c2"}


def test_other_workloads_are_the_baseline_configs_and_the_additive_joint():
    """The default one-GPU line of a --full run carries every BASELINE configuration and the additive joint:
    the key set is part of the contract with whoever reads BENCH_rNN.json."""
    sys.path.insert(0, ROOT)
    import bench
    assert set(bench.OTHER_WORKLOADS) | set(bench.ADD_WORKLOADS) | set(bench.MODULE_WORKLOADS) == EXPECTED_OTHER
    assert bench.WORKLOADS["c5_full"]["N"] == 1024 and bench.WORKLOADS["c5_full"]["dtype"] == "bf16"
    assert {bench.WORKLOADS[v]["dtype"] for v in bench.OTHER_WORKLOADS.values()} == {"fp32", "bf16"}


@pytest.mark.gpu
def test_default_line_carries_every_workload_with_a_passing_check():
    """`python bench.py --gpus 1 --full` (few steps; the CPU baseline and the PMC passes are the headline's and are covered by the
    driver's own --full run): c3 stays value / roofline, `other_workloads` has the ten entries, each with ms_per_step, its
    stage times, a roofline fraction and a check against the oracle that PASSED."""
    import json
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--no-traffic-pass"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["config"]["workload"].startswith("c3") and rec["check"]["passed"] and rec["roofline"]["frac"] > 0.5
    assert rec["check"]["max_err_over_quantum"] <= 1.0 and rec["check"]["max_rel_grad_err"] <= 1e-3
    other = rec["other_workloads"]
    assert set(other) == EXPECTED_OTHER
    for key, e in other.items():
        assert e["ms_per_step"] > 0 and e["step_ms"]["p10"] <= e["step_ms"]["median"] <= e["step_ms"]["p90"], key
        assert (e.get("stage_ms") or key.startswith("rnntloss_")) and e["path_frac"] > 0, key
        assert e["check"]["passed"], (key, e["check"])
        # the per-element keys: error / (one rounding of the stored value + fp32 arithmetic) <= 1
        assert 0 < e["check"]["max_err_over_quantum"] <= 1.0 and e["check"]["max_rel_grad_err"] < 5e-3, (key, e["check"])
        assert ("roofline" in e) or ("mfma_roofline" in e) or key.startswith("rnntloss_"), key
    assert rec["other_workloads_all_checks_passed"]
    assert other["c5_full_1024_on_one_gpu"]["ms_per_step"] > 4 * other["c5_per_gpu"]["ms_per_step"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only contract")
def test_full_is_an_option_of_every_command_line():
    """--full parses (alone and beside the options that trim it) and the run then ends where every run without a GPU ends."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                          "--no-cpu-baseline", "--no-traffic-pass", "--no-extra", "--no-verify"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 2 and not out.stdout.strip()
    assert "MI355X" in out.stderr and "usage:" not in out.stderr


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone():
    """`python bench.py --gpus 1 --steps N --warmup W` without --full: one line with the headline keys and the figures of the
    timed steps themselves, nothing that takes work of its own (no oracle check, CPU baseline, profiler pass, other workload),
    and at most 30 s of the whole process outside its N + W steps."""
    import json
    import math
    import time
    steps, warmup = 5, 2
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         capture_output=True, text=True, timeout=900)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"].startswith("ms/batch") and rec["unit"] == "ms/batch" and rec["higher_is_better"] is False
    assert rec["dtype"] == "f32" and rec["config"]["workload"].startswith("c3") and rec["n_gpus"] == 1
    assert rec["value"] == rec["ms_per_step"] > 0 and rec["steps"] == steps and rec["warmup"] == warmup and rec["step_ms"]["n"] == steps
    assert rec["stage_ms"]["grad"] > 0 and rec["roofline"]["frac"] > 0.5 and rec["path_roofline"]["frac"] > 0
    assert math.isfinite(rec["check"]["loss_sum"]) and "passed" not in rec["check"] and "samples_checked" not in rec["check"]
    assert "other_workloads" not in rec and "cpu_baseline" not in rec and rec["plain_step_ms"] is None
    assert "measured for this run" not in (rec["roofline"]["traffic_source"] or "")
    outside = wall - (steps + warmup) * rec["ms_per_step"] * 1e-3
    print("plain run: %.2f s wall clock, %.2f s outside its steps" % (wall, outside))
    assert outside <= 30.0, outside


def _dumped(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_files_and_sample(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files only, under 64 MB, with the gradient sample at the same indices
    on every call: small gradients whole, large ones as a seeded sample with its flat indices."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    costs = torch.rand(3, generator=g)
    small = torch.rand((3, 4, 5, 6), generator=g)
    bench.dump_outputs(str(tmp_path / "s"), costs, small)
    s = _dumped(tmp_path / "s")
    assert set(s) == {"costs", "grads", "grads_sq_sum"}
    assert np.array_equal(s["costs"], costs.numpy()) and np.array_equal(s["grads"], small.numpy())
    assert np.allclose(s["grads_sq_sum"], (small.double() ** 2).sum(dim=(1, 2, 3)).numpy())
    big = torch.rand((2, bench.DUMP_SAMPLE), generator=g).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), costs, big, reduced=torch.tensor([1.5, 3.0], dtype=torch.float64))
    a, b = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert set(a) == {"costs", "grads_sample", "grads_sample_index", "grads_sq_sum", "loss_reduced"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["grads_sample_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < big.numel() and len(idx) > bench.DUMP_SAMPLE // 2
    assert np.array_equal(a["grads_sample"], big.float().reshape(-1).numpy()[idx])


@pytest.mark.gpu
def test_dump_outputs_repeat_and_steps(tmp_path):
    """Two runs with the same arguments dump the same outputs (seeded inputs); the line reports the --steps asked for, and
    its per-step record holds exactly that many timed steps."""
    import json
    import numpy as np
    recs = []
    for d, steps in (("a", "3"), ("b", "4")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2", "--steps", steps,
                              "--warmup", "1", "--no-cpu-baseline", "--no-traffic-pass", "--dump-outputs", str(tmp_path / d)],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        recs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    assert [r["steps"] for r in recs] == [3, 4] and [r["step_ms"]["n"] for r in recs] == [3, 4]
    a, b = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert set(a) == set(b) and {"costs", "grads_sq_sum"} <= set(a)
    assert a["costs"].shape == (16,) and np.isfinite(a["costs"]).all()
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-6, atol=1e-7), k
