#!/usr/bin/env python
"""bench.py -- RNN-T loss+grad hot path on MI355X: ms/batch and fraction of the HBM roofline.

Contract (driver):  python bench.py --gpus N --steps K --warmup W.  Rank 0 prints ONE JSON line.
N>1: one rank per GPU over RCCL.  Either the driver launches the ranks itself
(python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N: WORLD_SIZE is set and must
equal N), or a plain `python bench.py --gpus N` re-launches itself under torch.distributed.run on
127.0.0.1.  Fewer than N visible devices is an error (exit code 2) -- never a silent 1-GPU run.
N=1 defaults to c3 (the headline configuration).  N>1 defaults to BASELINE config 5 AT EVERY N: the fixed global batch
of 1024 samples (T=200, U=41, A=1024, bf16) split N ways (512 / 256 / 128 per GPU; "scaling": "strong"); rank 0 also times
the whole 1024-sample batch on its own GPU once, so the line carries its own speed-up.  --per-gpu-batch B keeps the weak
form (B samples per GPU, global batch B*N).  --oversubscribe-gloo (development / single-GPU boxes) lets the ranks share the
visible device(s) over the gloo backend so that the launcher, the per-rank gather and the rank-0-only JSON line can run
where RCCL -- one rank per device -- cannot.

A "step" = one pass of the hot path over one synthetic batch already resident in HBM:
`compute_rnnt_loss` of include/rnnt.h with gradients (row statistics -> lattice -> coefficients
-> gradient write-back), i.e. exactly what the reference's tests/test_time.cu times
(compute_rnnt_loss incl. the costs D2H copy and stream sync).  With N>1 the batch is sharded
(contiguous slabs of samples, one per rank) and each step adds the single RCCL
all-reduce of the summed loss; the line then carries `multi_gpu` (ranks the backend saw, per-rank ms, the same
per-GPU shard timed without the collective, the whole global batch on one GPU, speed-up and efficiency).

A plain run does only what the headline needs: set up, warm up, time the steps, dump, print.  Its line has the headline keys, the
per-step and per-stage times of those very steps (and the rooflines derived from them, `roofline.traffic` from the committed
profiles), and `check.loss_sum`.  --full adds everything that takes work of its own: `check` = two samples of the timed batch
against the fp64 oracle (outside the timed region; --no-verify skips it), `cpu_baseline` (--no-cpu-baseline), `roofline.traffic`
measured for the run by two profiler passes (--no-traffic-pass), `plain_step_ms` (sub-0.5 ms steps once more without the stage
events) and, on a default one-GPU line, `other_workloads` (--no-extra).  The --no-* options only subtract from --full.
(N > 1 lines keep `multi_gpu` whole with or without --full: the shard without the collective and the whole batch on one GPU
are what that line's speed-up and efficiency are read against; --no-full-batch trims them.)
--dump-outputs DIR writes what the headline's last timed step returned (costs, gradients or a fixed sample of them) as
.npy files: the inputs are seeded, so two builds run with the same arguments can be compared output for output.

Workloads (BASELINE.json configs; lattice U = L+1 as tests/test_time.cu:56):
  c2: N=16  T=150  L=40  A=28   fp32      c3: N=128 T=150 L=20 A=5000 fp32  (default, headline)
  c4: N=64  T=1500 L=300 A=50   fp32      c5: T=200 L=40 A=1024 bf16, global batch 1024 over N GPUs (one GPU: 128)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "warp-transducer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

WORKLOADS = {
    "c2": dict(N=16, T=150, L=40, A=28, dtype="fp32", published_ms=11.43),
    "c3": dict(N=128, T=150, L=20, A=5000, dtype="fp32", published_ms=51.46),
    "c4": dict(N=64, T=1500, L=300, A=50, dtype="fp32", published_ms=None),
    "c5": dict(N=128, T=200, L=40, A=1024, dtype="bf16", published_ms=None),
    "c5_full": dict(N=1024, T=200, L=40, A=1024, dtype="bf16", published_ms=None),   # BASELINE config 5 whole, on ONE GPU (8.6e9 elements)
}
# Every default one-GPU line of a --full run also carries these, each with its own oracle check (`other_workloads`; --no-extra skips them):
# the BASELINE configurations the headline is not quoted on, config 5 whole on one GPU (the base the N > 1 lines' strong
# scaling is read against -- the SAME key appears in those lines), and the additive joint.
OTHER_WORKLOADS = {"c2": "c2", "c4": "c4", "c5_per_gpu": "c5", "c5_full_1024_on_one_gpu": "c5_full"}
ADD_WORKLOADS = {"add_c3_f32": ("c3", "fp32"), "add_c3_bf16": ("c3", "bf16"), "add_c4_f32": ("c4", "fp32")}
# ... and the wrapper north_star names: warprnnt_pytorch.RNNTLoss forward + backward through autograd (the compiled extension
# module), what the reference's pytorch_binding/test/test_time.py:45-80 times
MODULE_WORKLOADS = {"rnntloss_c3": "c3", "rnntloss_c5": "c5", "rnntloss_c2": "c2"}
MFMA_PEAK_TFLOPS = {"fp32": 157.3, "bf16": 2500.0}   # dense matrix-core peaks (MI355X_MICROARCH.md)
SHARDED_GLOBAL_BATCH = {"c5": 1024}   # BASELINE config 5: N=1024 sharded over the GPUs of one node (other workloads: their own N)
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md)
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp64": torch.float64, "fp16": torch.float16}
ESIZE = {"fp32": 4, "bf16": 2, "fp64": 8, "fp16": 2}


def make_inputs(w, dev, seed):
    """Synthetic batch of the reference timing harness's shape (tests/test_time.cu:27-62): logits
    uniform(0,1), every sample full length, labels in [1, A-1] with forced repeats, blank 0.
    Generated on the device (the host mt19937 stream takes ~1 min at c3 size: BASELINE.md 3)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    N, T, L, A = w["N"], w["T"], w["L"], w["A"]
    U = L + 1
    acts = torch.empty((N, T, U, A), device=dev, dtype=TORCH_DT[w["dtype"]])
    for b0 in range(0, N, 128):        # in slabs: the fp32 draw of the whole config-5 batch would be 34 GB of temporary
        acts[b0:b0 + 128] = torch.rand((min(128, N - b0), T, U, A), generator=g, device=dev, dtype=torch.float32).to(acts.dtype)
    lab = torch.randint(1, A, (L,), generator=g, device=dev, dtype=torch.int32)
    if L >= 3:
        lab[L // 2] = lab[L // 2 + 1]
        lab[L // 2 - 1] = lab[L // 2]
    labels = lab.unsqueeze(0).repeat(N, 1).contiguous()
    act_lens = torch.full((N,), T, dtype=torch.int32, device=dev)
    label_lens = torch.full((N,), L, dtype=torch.int32, device=dev)
    return acts, labels, act_lens, label_lens


def algorithmic_bytes(w, valid_rows=None, packed=False):
    """acts read twice, grads written once, plus the fp32 lattice side arrays.
    With variable lengths only the valid (t < T_b, u < U_b) rows have to be READ; every row of
    the gradient tensor is still written (zeros in the padding) -- unless the layout is packed,
    where the padding does not exist."""
    N, T, U, A, s = w["N"], w["T"], w["L"] + 1, w["A"], ESIZE[w["dtype"]]
    R = N * T * U
    Rv = R if valid_rows is None else valid_rows
    if packed:
        R = Rv
    E, Ev = R * A, Rv * A
    return dict(E=E, R=R, path=2 * Ev * s + E * s + 48 * Rv, grad_kernel=Ev * s + E * s + 16 * R,
                stats_kernel=Ev * s + 16 * Rv)


def cpu_model():
    """The host CPU's model string (core count AND model stated next to the CPU baseline)."""
    try:
        names = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.lower().startswith("model name")]
        if names:
            sockets = len({l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.lower().startswith("physical id")}) or 1
            return "%s (%d logical CPUs, %d socket(s))" % (names[0], len(names), sockets)
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine() or "unknown"


def cpu_topology():
    """Logical CPUs, physical cores and threads per core of the host, and how the baseline's OpenMP threads are placed
    (`cores: 128` next to a 256-CPU host must say which 128)."""
    logical = os.cpu_count() or 1
    cores = set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip() and phys is not None and core is not None:
                cores.add((phys, core)); phys = core = None
    except OSError:
        pass
    physical = len(cores) or logical
    try:
        allowed = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        allowed = logical
    return {"logical_cpus": logical, "physical_cores": physical, "threads_per_core": max(1, logical // max(physical, 1)),
            "cpus_this_process_may_use": allowed,
            "omp_places": os.environ.get("OMP_PLACES", "(unset)"), "omp_proc_bind": os.environ.get("OMP_PROC_BIND", "(unset)"),
            "placement": "not pinned: the OpenMP runtime's threads float, the kernel scheduler spreads them over idle cores first "
                         "(with fewer threads than physical cores no SMT sibling has to be shared)"}


def cpu_baseline(w, acts, labels, act_lens, label_lens, budget_samples):
    """The REFERENCE's own CPU path (oracle/_ref, compiled from /root/reference) on the host
    cores of this box, on a bounded sample of the same workload (last row).  Three legs:
      value             all host cores, the reference CPU contract (log-probs in, sparse log-prob
                        gradients out: log_softmax is NOT in its time) -- tests/test_time.cpp's measurement
      single_thread     the same call with num_threads = 1 on a smaller slice
      with_log_softmax  like for like with the GPU path (logits in, dense logit gradients out):
                        torch.log_softmax forward + the reference call + log_softmax backward, all cores"""
    from oracle import oracle as O
    N = w["N"]
    n = min(N, budget_samples)
    x = torch.cat([acts[i:i + 16].float().cpu() for i in range(0, n, 16)])
    lp_t = torch.log_softmax(x, -1)
    lp = lp_t.numpy()
    lab, tl, ll = labels[:n].cpu().numpy(), act_lens[:n].cpu().numpy(), label_lens[:n].cpu().numpy()
    cores = os.cpu_count() or 1
    threads = min(cores, n)
    if O.have_ref():
        kind = "reference"

        def call(lpa, k, nthreads, want_grads=False):
            return O.ref_rnnt_logprobs(lpa[:k], lab[:k], tl[:k], ll[:k], 0, True, nthreads)
    else:
        kind = "port"

        def call(lpa, k, nthreads, want_grads=False):
            O.lib().oracle_set_num_threads(nthreads)
            return O.rnnt_logprobs(lpa[:k], lab[:k], tl[:k], ll[:k], 0, True)

    def timed(fn, reps=3):
        fn()   # page-fault warm-up (the reference harness pays it inside its timing: BASELINE.md 3)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times))

    ms_all = timed(lambda: call(lp, n, threads)) * (N / n)
    # steady state: the same call, same threads, with the gradient / workspace / cost buffers allocated and
    # touched ONCE outside the timing -- the figure above re-allocates them per call (as tests/test_time.cpp:57-60 does) and
    # is dominated by first-touch page faults of a fresh gradient array
    steady = None
    if kind == "reference":
        prepared = O.RefCall(lp[:n], lab[:n], tl[:n], ll[:n], 0, threads)
        ms_steady = timed(prepared, reps=5) * (N / n)
        c_chk, _ = call(lp, min(n, 4), threads)
        assert np.allclose(prepared.costs[:min(n, 4)], c_chk, rtol=1e-6)
        n1s = max(1, min(n, int(n * 4000.0 / max(ms_steady * (n / N) * threads, 1.0))))
        prepared1 = O.RefCall(lp[:n1s], lab[:n1s], tl[:n1s], ll[:n1s], 0, 1)
        ms_steady1 = timed(prepared1, reps=2) * (N / n1s)
        steady = dict(value=round(ms_steady, 3), unit="ms/batch", cores=threads,
                      sample="%d of %d samples, gradient / workspace / cost buffers allocated once and first touched by an untimed call of the "
                             "reference itself (each OpenMP thread faults in its own samples' slabs), median of 5 warmed calls, scaled x%.2f" % (n, N, N / n),
                      single_thread=dict(value=round(ms_steady1, 3), unit="ms/batch", cores=1,
                                         sample="%d of %d samples, same protocol, median of 2, scaled x%.2f" % (n1s, N, N / n1s)))
        del prepared, prepared1
    # one thread: a slice sized to a few seconds (the whole-batch call above took ms_all on `threads` threads)
    n1 = max(1, min(n, int(n * 4000.0 / max(ms_all * (n / N) * threads, 1.0))))
    ms_one = timed(lambda: call(lp, n1, 1), reps=2) * (N / n1)

    # like for like: logits -> loss + dense logit gradients
    n2 = min(n, 32)
    torch.set_num_threads(threads)

    def full():
        xx = x[:n2].clone().requires_grad_(True)
        l = torch.log_softmax(xx, -1)
        _, g_lp = call(l.detach().numpy(), n2, min(threads, n2))
        l.backward(torch.from_numpy(np.ascontiguousarray(g_lp)))
        return xx.grad
    ms_full = timed(full, reps=2) * (N / n2)
    shape = "T=%d,U=%d,A=%d" % (w["T"], w["L"] + 1, w["A"])
    return dict(value=round(steady["value"] if steady else ms_all, 3), unit="ms/batch", cores=threads, cpu_model=cpu_model(), kind=kind,
                host=cpu_topology(),
                protocol=("steady_state (buffers pre-touched); the reference harness's own protocol is `harness_protocol`" if steady
                          else "harness_protocol"),
                steady_state=steady,
                harness_protocol=dict(value=round(ms_all, 3), unit="ms/batch", cores=threads,
                                      sample="fresh gradient / workspace arrays per call, as tests/test_time.cpp:57-60: first-touch "
                                             "page faults inside the timing; median of 3, scaled x%.2f" % (N / n)),
                threads_note="one OpenMP thread per sample -- the reference parallelises over the batch only (cpu_rnnt.h:290), so a batch "
                             "of %d samples can occupy at most %d threads whatever the host has" % (n, n),
                sample="%d of %d samples (%s, fp32 log-probs in, sparse log-prob grads out), "
                       "median of 3 warmed calls, scaled x%.2f to the full batch; host has %d cores"
                       % (n, N, shape, N / n, cores),
                single_thread=dict(value=round(ms_one, 3), unit="ms/batch", cores=1,
                                   sample="%d of %d samples, median of 2 warmed calls, scaled x%.2f" % (n1, N, N / n1)),
                with_log_softmax=dict(value=round(ms_full, 3), unit="ms/batch", cores=threads,
                                      sample="%d of %d samples: torch.log_softmax forward + reference CPU call + "
                                             "log_softmax backward (logits in, dense logit grads out, the GPU "
                                             "path's contract), median of 2 warmed calls, scaled x%.2f"
                                             % (n2, N, N / n2)))


def measure_traffic(argv_tail, kernel="grad_flat_kernel"):
    """HBM bytes per launch of the dominant kernel, MEASURED for this command on this box: two extra passes of the same
    workload (3 steps) under `rocprofv3 --pmc FETCH_SIZE --kernel-trace` and `--pmc WRITE_SIZE --kernel-trace` (separate
    passes, counters in their own runs, as MI355X_MICROARCH.md's HBM section prescribes), FETCH_SIZE doubled (that guide's
    gfx950 correction for wide coalesced reads), both counters in KiB.  Outside the timed region; None if rocprofv3 is
    not there or a pass fails (the committed profiles/ figure is reported then, and labelled so)."""
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from make_traffic import per_launch
    except ImportError:
        return None
    got = {}
    tmp = None
    try:
        tmp = tempfile.mkdtemp(prefix="rnnt_pmc_", dir="/tmp" if os.path.isdir("/tmp") else None)
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out_dir = os.path.join(tmp, ctr)
            cmd = [prof, "--pmc", ctr, "--kernel-trace", "-d", out_dir, "-o", "pmc", "--", sys.executable,
                   os.path.abspath(__file__)] + argv_tail + ["--steps", "3", "--warmup", "1"]     # (a plain run: the steps alone)
            r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, TMPDIR=tmp), capture_output=True, text=True, timeout=600)
            dbs = glob.glob(os.path.join(out_dir, "**", "*.db"), recursive=True)
            if r.returncode != 0 or not dbs:
                return None
            per = per_launch(dbs[0], ctr)
            hit = [v for k, v in per.items() if kernel in k]
            if not hit:
                return None
            got[ctr] = hit[0]
    except (OSError, subprocess.SubprocessError, ValueError, KeyError, Exception):       # noqa: BLE001 -- measurement aid only
        return None
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)
    return int((2 * got["FETCH_SIZE"] + got["WRITE_SIZE"]) * 1024)


class _NcclUniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]               # rccl.h: NCCL_UNIQUE_ID_BYTES


def native_communicator(world, rank, dev, timeout_s=120.0):
    """An RCCL communicator of this job's ranks for compute_rnnt_loss_sharded (the library issues the collective itself):
    rank 0 draws the unique id, torch.distributed broadcasts its 128 bytes, every rank joins.  (None, None) when RCCL
    cannot be loaded or the communicator cannot be formed ON ANY RANK -- the ranks agree on the outcome through one
    torch.distributed all-reduce, so that no rank issues the native collective while another waits in torch's -- and the
    step then uses torch.distributed's all-reduce everywhere.  The join runs in a helper thread with a time limit: a
    bootstrap that never returns costs the native path, not the run."""
    import threading
    state = {"rccl": None, "comm": None, "why": None}
    try:
        rccl = None
        for name in ("librccl.so.1", "librccl.so"):
            try:
                rccl = C.CDLL(name)
                break
            except OSError:
                continue
        if rccl is None:
            state["why"] = "librccl not loadable"
        else:
            rccl.ncclGetUniqueId.argtypes = [C.POINTER(_NcclUniqueId)]
            rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, _NcclUniqueId, C.c_int]
            rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        uid = _NcclUniqueId()
        if rccl is not None and rank == 0 and rccl.ncclGetUniqueId(C.byref(uid)) != 0:
            state["why"] = "ncclGetUniqueId failed"
        # (every rank takes part in the broadcast, whatever happened above: the collectives of the ranks must pair up)
        raw = torch.frombuffer(bytearray(C.string_at(C.addressof(uid), 128)), dtype=torch.uint8).to(dev)   # (all 128 bytes: a c_char field reads as a NUL-terminated string)
        if world > 1:
            dist.broadcast(raw, src=0)
        C.memmove(C.byref(uid), bytes(raw.cpu().numpy().tobytes()), 128)
        if rccl is not None and state["why"] is None:
            def join():
                try:
                    torch.cuda.set_device(dev)
                    comm = C.c_void_p()
                    rc = rccl.ncclCommInitRank(C.byref(comm), world, uid, rank)
                    if rc == 0:
                        state["comm"] = comm
                    else:
                        state["why"] = "ncclCommInitRank failed (%d)" % rc
                except Exception as e:                             # noqa: BLE001
                    state["why"] = repr(e)
            th = threading.Thread(target=join, daemon=True)
            th.start()
            th.join(timeout_s)
            if th.is_alive():
                state["why"] = "ncclCommInitRank did not return within %.0f s" % timeout_s
                state["comm"] = None
            state["rccl"] = rccl
    except Exception as e:                                         # noqa: BLE001 -- fall back to torch.distributed's collective
        state["why"] = repr(e)
        state["comm"] = None
    if state["comm"] is not None:
        # Introduce the communicator to the library HERE, before the ranks agree: the library must call the ncclAllReduce of
        # the RCCL copy that made `comm` (say which, do not let it guess), and rnnt_sharded_prepare resolves it now -- a rank
        # on which that fails votes "no" below instead of failing in front of a collective its peers have entered.
        from warprnnt_pytorch import _lib as _wl
        _wl.lib().rnnt_set_rccl_all_reduce(C.cast(state["rccl"].ncclAllReduce, C.c_void_p))
        if _wl.lib().rnnt_sharded_prepare(state["comm"]) != 0:
            state["why"] = "rnnt_sharded_prepare failed (no unambiguous RCCL in this process)"
            state["rccl"].ncclCommDestroy(state["comm"])
            state["comm"] = None
    ok = torch.tensor([1 if state["comm"] is not None else 0], dtype=torch.int32, device=dev)
    if world > 1:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        if state["comm"] is not None:                              # another rank could not join: nobody uses the native path
            _wl.lib().rnnt_sharded_release(state["comm"])
            state["rccl"].ncclCommDestroy(state["comm"])
        print("bench.py: no native RCCL communicator on rank %d (%s); every rank uses torch.distributed's all-reduce"
              % (rank, state["why"] or "another rank could not join"), file=sys.stderr)
        return None, None
    return state["rccl"], state["comm"]


DUMP_SAMPLE = 1 << 22     # --dump-outputs: gradient elements kept of a larger gradient (16 MB fp32 + 32 MB fp64 indices)


def dump_outputs(path, costs, grads, reduced=None):
    """--dump-outputs DIR: what the timed path handed its caller in the LAST timed step, as DIR/<name>.npy, so that two
    builds can be compared output for output (the inputs are seeded: the same arguments give the same batch).
      costs.npy               (N,) float32     the per-sample costs
      grads.npy               float32          the whole gradient tensor, when it has at most DUMP_SAMPLE elements; else
      grads_sample.npy        (k,) float32     a fixed sample of it (seed 0, sorted flat indices, the same for every run) and
      grads_sample_index.npy  (k,) float64     those flat indices (exact in float64)
      grads_sq_sum.npy        (grads.shape[0],) float64   sum of squares over every axis but the first (covers every element)
      loss_reduced.npy        float64          sharded runs: the all-reduced loss this rank received"""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "costs.npy"), costs.detach().float().cpu().numpy())
    flat = grads.detach().reshape(-1)
    n = flat.numel()
    if n <= DUMP_SAMPLE:
        np.save(os.path.join(path, "grads.npy"), flat.float().cpu().numpy().reshape(tuple(grads.shape)))
    else:
        idx = np.unique(np.random.default_rng(0).integers(0, n, DUMP_SAMPLE, dtype=np.int64))
        np.save(os.path.join(path, "grads_sample.npy"), flat[torch.from_numpy(idx).to(flat.device)].float().cpu().numpy())
        np.save(os.path.join(path, "grads_sample_index.npy"), idx.astype(np.float64))
    g2 = grads.detach().reshape(grads.shape[0], -1)
    rows = max(1, (1 << 26) // max(1, g2.shape[1]))                 # fp64 temporaries of at most 512 MB
    sq = torch.cat([g2[i:i + rows].double().square().sum(dim=1) for i in range(0, g2.shape[0], rows)])
    np.save(os.path.join(path, "grads_sq_sum.npy"), sq.cpu().numpy())
    if reduced is not None:
        np.save(os.path.join(path, "loss_reduced.npy"), reduced.detach().double().cpu().numpy())


def verify_batch(w, acts, labels, act_lens, label_lens, grads, costs, acts_picked=None):
    """Parity evidence for THIS run, outside the timed region: the first and the last sample of the timed batch (the
    gradients and costs the last timed step left behind) against the fp64 oracle on the same -- storage-rounded --
    inputs.  Loss: north_star's 1e-4, relative.  Gradients: north_star's 1e-3 absolute (bf16 storage: 4e-3) is kept, but at
    A = 5000 / 1024 it exceeds every non-blank / non-label entry, so the deciding bound is per element (oracle.grad_bound):
    |got - ref| <= q |ref| + r mag + a, q = one rounding of the stored value (2^-8 bf16, 0 fp32), r mag = the fp32 arithmetic
    ahead of it relative to the terms of the element (1e-3 fp32, 2^-13 bf16), a = 1e-5 / 2e-6.  `max_err_over_quantum` is
    the largest error / bound (<= 1 passes), `max_rel_grad_err` the largest error / terms."""
    from oracle import oracle as O
    N = acts.shape[0]
    pick = sorted({0, N - 1})
    xs = (acts[pick] if acts_picked is None else acts_picked).double().cpu().numpy()     # (in-place runs: the logits are gone)
    O.lib().oracle_set_num_threads(min(len(pick), os.cpu_count() or 1))
    ref_c, ref_g, mag = O.rnnt_logits(xs, labels[pick].cpu().numpy(), act_lens[pick].cpu().numpy(), label_lens[pick].cpu().numpy(),
                                      want_mag=True)
    got_c = costs[pick].double().cpu().numpy()
    got_g = grads[pick].double().cpu().numpy()
    rel = float((np.abs(got_c - ref_c) / np.maximum(1.0, np.abs(ref_c))).max())
    tol_g = 1e-3 if w["dtype"] == "fp32" else 4e-3
    chk = O.grad_check(got_g, ref_g, mag, w["dtype"])
    return {"samples_checked": pick, "max_rel_loss_err": rel, "max_abs_grad_err": chk["max_abs_grad_err"],
            "max_rel_grad_err": chk["max_rel_grad_err"], "max_err_over_quantum": chk["max_err_over_quantum"],
            "tolerance": {"loss_rel": 1e-4, "grad_abs": tol_g,
                          "grad_per_element": "|got-ref| <= %.3g*|ref| + %.3g*terms + %.0e (oracle.grad_bound)"
                                              % (O.QUANTUM[w["dtype"]], O._REL[w["dtype"]], O._ABS[w["dtype"]])},
            "passed": bool(rel <= 1e-4 and chk["max_abs_grad_err"] <= tol_g and chk["passed"]),
            "against": "oracle/ (fp64 restatement of the reference CPU path) on the same inputs, outside the timed region"}


def run_rnntloss_workload(dev, key, steps, warmup, verify=True):
    """`RNNTLoss(reduction='mean')(acts, labels, act_lens, label_lens)` + `loss.backward()` + one device sync per step: the
    module of /root/reference/pytorch_binding/warprnnt_pytorch/__init__.py:82-141 as its test_time.py:45-80 drives it.  The
    gradient the autograd engine leaves in `acts.grad` (scaled by 1/N) is what the check judges, against the oracle on two
    samples of the timed batch; the timed mean loss against the per-sample costs of an untimed reduction='none' call."""
    from warprnnt_pytorch import RNNTLoss, warp_rnnt
    w = WORKLOADS[MODULE_WORKLOADS[key]]
    acts, labels, act_lens, label_lens = make_inputs(w, dev, 4242)
    N, T, U, A = acts.shape
    acts.requires_grad_(True)
    crit = RNNTLoss(blank=0, reduction="mean")
    state = {}

    def step():
        acts.grad = None
        loss = crit(acts, labels, act_lens, label_lens)
        loss.backward()
        torch.cuda.synchronize(dev)
        state["loss"] = loss

    for _ in range(warmup):
        step()
    t0 = time.perf_counter()
    marks = []
    for _ in range(steps):
        step()
        marks.append(time.perf_counter())
    per_step = np.diff(np.array([t0] + marks)) * 1e3
    ms = float(per_step.mean())
    s = ESIZE[w["dtype"]]
    ab = algorithmic_bytes(w)
    rec = {"workload": "warprnnt_pytorch.RNNTLoss(reduction='mean') forward + loss.backward() + device sync, %s: N=%d T=%d U=%d A=%d %s, "
                       "binding: %s" % (MODULE_WORKLOADS[key], N, T, U, A, w["dtype"], warp_rnnt.binding()),
           "ms_per_step": round(ms, 4),
           "step_ms": dict(median=round(float(np.median(per_step)), 4), p10=round(float(np.percentile(per_step, 10)), 4),
                           p90=round(float(np.percentile(per_step, 90)), 4), n=int(per_step.size)),
           "path_frac": round(ab["path"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "bytes_algo": ab["path"],
           "note": "two-phase entries under autograd: forward = statistics + lattice + coefficients, backward = the one gradient pass "
                   "with grad_output / N folded in (the reference's module keeps and rescales a (N,T,U,A) tensor)"}
    if verify:
        from oracle import oracle as O
        pick = sorted({0, N - 1})
        with torch.no_grad():
            per_sample = RNNTLoss(blank=0, reduction="none")(acts.detach(), labels, act_lens, label_lens).double().cpu().numpy()
        O.lib().oracle_set_num_threads(min(len(pick), os.cpu_count() or 1))
        ref_c, ref_g, mag = O.rnnt_logits(acts.detach()[pick].double().cpu().numpy(), labels[pick].cpu().numpy(),
                                          act_lens[pick].cpu().numpy(), label_lens[pick].cpu().numpy(), want_mag=True)
        rel = float((np.abs(per_sample[pick] - ref_c) / np.maximum(1.0, np.abs(ref_c))).max())
        mean_rel = abs(float(state["loss"].item()) - per_sample.mean()) / abs(per_sample.mean())
        chk = O.grad_check(acts.grad[pick].double().cpu().numpy(), ref_g / N, mag / N, w["dtype"], scale=1.0 / N)
        rec["check"] = {"samples_checked": pick, "max_rel_loss_err": rel, "mean_loss_vs_per_sample_costs_rel": mean_rel,
                        "max_abs_grad_err": chk["max_abs_grad_err"], "max_rel_grad_err": chk["max_rel_grad_err"],
                        "max_err_over_quantum": chk["max_err_over_quantum"],
                        "passed": bool(rel <= 1e-4 and mean_rel <= 1e-5 and chk["passed"]),
                        "against": "oracle/ (fp64) on the same inputs; acts.grad (= gradient / N) per element, oracle.grad_bound"}
    del acts, state
    torch.cuda.empty_cache()
    return rec


def run_add_workload(lib, dev, name, steps, warmup, verify=True):
    """The additive joint (compute_rnnt_loss_add*: f (N,T,A) + g (N,U,A), the (N,T,U,A) tensor never exists) on a BASELINE
    shape: one step = forward + both gradients, enqueue + device sync.  Checked against the fp64 oracle on the MATERIALISED
    joint of two samples (outside the timed region).  Rooflines: the three contractions (partition function, df, dg) are
    3 * 2*N*T*U*A matrix-core flops; HBM bytes = f and g read by the forward and by the backward phase + df, dg written +
    the lattice side arrays (48 B per cell)."""
    from warprnnt_pytorch import _lib
    shape_of, dtype = ADD_WORKLOADS[name]
    w = WORKLOADS[shape_of]
    N, T, L, A = w["N"], w["T"], w["L"], w["A"]
    U = L + 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    tdt = TORCH_DT[dtype]
    f = torch.rand((N, T, A), generator=gen, device=dev).to(tdt)
    g = torch.rand((N, U, A), generator=gen, device=dev).to(tdt)
    lab = torch.randint(1, A, (L,), generator=gen, device=dev, dtype=torch.int32)
    labels = lab.unsqueeze(0).repeat(N, 1).contiguous()
    tl = torch.full((N,), T, dtype=torch.int32, device=dev)
    ll = torch.full((N,), L, dtype=torch.int32, device=dev)
    df, dg = torch.empty_like(f), torch.empty_like(g)
    costs = torch.zeros(N, dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.workspace_bytes_add(T, U, N), dtype=torch.uint8, device=dev)
    opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream, blank_label=0,
                           maxT=T, maxU=U, batch_first=True)
    code = {"fp32": _lib.DT_F32, "bf16": _lib.DT_BF16}[dtype]
    fwd = (f.data_ptr(), g.data_ptr(), labels.data_ptr(), ll.data_ptr(), tl.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(), opt, code, 1, 0.0)
    bwd = (f.data_ptr(), g.data_ptr(), df.data_ptr(), dg.data_ptr(), None, labels.data_ptr(), ll.data_ptr(), tl.data_ptr(), A, N,
           ws.data_ptr(), opt, code)

    def step():
        st = lib.compute_rnnt_loss_add_fwd_dt(*fwd)
        assert st == 0, _lib.status_string(st)
        st = lib.compute_rnnt_loss_add_bwd_dt(*bwd)
        assert st == 0, _lib.status_string(st)
        torch.cuda.synchronize(dev)
        lib.rnnt_profile_collect()

    for _ in range(warmup):
        step()
    lib.rnnt_profile_reset()
    lib.rnnt_profile_enable(1)
    t0 = time.perf_counter()
    marks = []
    for _ in range(steps):
        step()
        marks.append(time.perf_counter())
    lib.rnnt_profile_enable(0)
    per_step = np.diff(np.array([t0] + marks)) * 1e3
    ms = float(per_step.mean())
    stage = (C.c_double * 5)()
    calls = lib.rnnt_profile_read(stage, 5)
    s = ESIZE[dtype]
    flops = 3 * 2.0 * N * T * U * A
    hbm = 3 * (N * T * A + N * U * A) * s + 48 * N * T * U
    rec = {"workload": "additive joint f(N,T,A)+g(N,U,A), %s shape N=%d T=%d U=%d A=%d, %s storage: compute_rnnt_loss_add_fwd_dt + _bwd_dt "
                       "(costs, df, dg) + device sync" % (shape_of, N, T, U, A, dtype),
           "ms_per_step": round(ms, 4),
           "step_ms": dict(median=round(float(np.median(per_step)), 4), p10=round(float(np.percentile(per_step, 10)), 4),
                           p90=round(float(np.percentile(per_step, 90)), 4), n=int(per_step.size)),
           "stage_ms": ({"z_stats": round(stage[0] / calls, 4), "lattice": round(stage[1] / calls, 4), "coef": round(stage[2] / calls, 4),
                         "df_dg": round(stage[3] / calls, 4)} if calls else None),
           "mfma_roofline": {"bound": "mfma", "flops_algo": flops, "achieved": round(flops / (ms * 1e-3) / 1e12, 2),
                             "peak": MFMA_PEAK_TFLOPS[dtype], "unit": "TFLOP/s",
                             "frac": round(flops / (ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[dtype], 4),
                             "note": "three contractions of 2*N*T*U*A flops over the WHOLE step (lattice and coefficient kernels included)"},
           "path_frac": round(hbm / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "bytes_algo": hbm,
           "materialised_equivalent_bytes": 3 * N * T * U * A * s}
    # The bound that matters: these GEMMs are thin (U / 4 flop per byte) -- HBM, not the matrix cores.
    # Over the whole step; `traffic` = HBM bytes per step counted by the committed rocprofv3 --pmc passes per kernel
    # (tools/add_network_roofline.py --json; FETCH_SIZE calibrated for these kernels' load shapes: profiles/r06/fetch_calibration.md)
    rec["roofline"] = {"bound": "hbm", "achieved": round(hbm / (ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": rec["path_frac"], "bytes_algo": hbm, "traffic": None,
                       "note": "whole step (forward + backward phase, every kernel and launch gap) against 8 TB/s"}
    try:
        import glob
        tfile = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_add_traffic.json")))[-1]
        tj = json.load(open(tfile))[name]
        rec["roofline"]["traffic"] = tj["traffic_bytes_per_step"]
        rec["roofline"]["traffic_over_algorithmic"] = round(tj["traffic_bytes_per_step"] / hbm, 3)
        rec["roofline"]["traffic_source"] = "profiles/%s (committed rocprofv3 --pmc passes per kernel; not measured in this run)" % os.path.basename(tfile)
    except (OSError, KeyError, ValueError, IndexError):
        pass
    if verify:
        from oracle import oracle as O
        pick = sorted({0, N - 1})
        fr, gr = f[pick].double().cpu().numpy(), g[pick].double().cpu().numpy()
        O.lib().oracle_set_num_threads(min(len(pick), os.cpu_count() or 1))
        ref_c, ref_gz, mag = O.rnnt_logits(fr[:, :, None, :] + gr[:, None, :, :], labels[pick].cpu().numpy(), tl[pick].cpu().numpy(),
                                           ll[pick].cpu().numpy(), want_mag=True)
        rdf, rdg = ref_gz.sum(axis=2), ref_gz.sum(axis=1)
        mdf, mdg = mag.sum(axis=2), mag.sum(axis=1)                  # the terms a summed element is made of
        del ref_gz, mag
        rel = float((np.abs(costs[pick].double().cpu().numpy() - ref_c) / np.maximum(1.0, np.abs(ref_c))).max())
        # df sums U per-cell gradients, dg sums T of them: north_star's per-element 1e-3 is kept per SUMMED element
        # relative to the count (tests/test_gpu_add_network.py uses the same form); bf16 storage: + half an ulp of the stored value
        ulp = 5e-5 if dtype == "fp32" else 2.0 ** -8
        edf = np.abs(df[pick].double().cpu().numpy() - rdf) - ulp * np.abs(rdf)
        edg = np.abs(dg[pick].double().cpu().numpy() - rdg) - ulp * np.abs(rdg)
        tol_df, tol_dg = 2e-4 * max(1.0, U / 32), 2e-4 * max(1.0, T / 32)
        # the absolute figures above exceed most entries of df / dg at A = 5000; per element, relative to the summed terms
        # (the contraction runs on the matrix cores from factorised exponentials: 1e-3 of the terms for either storage type)
        cdf = O.grad_check(df[pick].double().cpu().numpy(), rdf, mdf, dtype, rel=1e-3)
        cdg = O.grad_check(dg[pick].double().cpu().numpy(), rdg, mdg, dtype, rel=1e-3)
        rec["check"] = {"samples_checked": pick, "max_rel_loss_err": rel, "max_abs_df_err": float(edf.max()), "max_abs_dg_err": float(edg.max()),
                        "max_abs_grad_err": max(cdf["max_abs_grad_err"], cdg["max_abs_grad_err"]),
                        "max_rel_grad_err": max(cdf["max_rel_grad_err"], cdg["max_rel_grad_err"]),
                        "max_err_over_quantum": max(cdf["max_err_over_quantum"], cdg["max_err_over_quantum"]),
                        "tolerance": {"loss_rel": 1e-4, "df_abs": tol_df, "dg_abs": tol_dg,
                                      "note": "absolute, after subtracting %.1e x |reference| (accumulation over U resp. T terms%s)"
                                              % (ulp, "" if dtype == "fp32" else "; bf16 storage quantum")},
                        "passed": bool(rel <= 1e-4 and edf.max() <= tol_df and edg.max() <= tol_dg and cdf["passed"] and cdg["passed"]),
                        "against": "oracle/ (fp64) on the MATERIALISED joint f_t + g_u of these samples, gradients summed over u / t"}
    del f, g, df, dg, ws
    torch.cuda.empty_cache()
    return rec


def main():
    # stdout carries the ONE JSON line and nothing else: whatever libraries print on the way (RCCL's version banner at
    # communicator creation goes to C stdout) is sent to stderr until the line is ready
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="default: c3 on one GPU (the headline configuration), c5 when --gpus > 1")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: the parity check against the fp64 oracle, the "
                         "CPU baseline, the profiler passes behind `roofline.traffic`, `plain_step_ms` and, on a default one-GPU "
                         "line, `other_workloads`.  Off by default: a plain run sets up, warms up, times, dumps and prints")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip `cpu_baseline`")
    ap.add_argument("--cpu-samples", type=int, default=128)
    ap.add_argument("--extra", action="store_true", help="with --full: `other_workloads` also beside an explicit --workload")
    ap.add_argument("--no-extra", action="store_true",
                    help="with --full, one GPU: skip `other_workloads` (c2, c4, c5 per GPU, config 5 whole on one GPU, additive joint)")
    ap.add_argument("--override", default="", help="dev: override workload fields, e.g. A=4992,N=64")
    ap.add_argument("--varlen", action="store_true",
                    help="robustness run: T_b ~ U[T/2,T], L_b ~ U[L/2,L] (seed 2, maxima forced), SURVEY.md 8d")
    ap.add_argument("--packed", action="store_true",
                    help="with --varlen: the same batch in the PACKED layout (compute_rnnt_loss_packed: no padded "
                         "rows in the tensors at all); single GPU")
    ap.add_argument("--pinned-costs", action="store_true",
                    help="host costs in pinned memory: the lattice kernel writes them directly, no staged D2H copy "
                         "(the default, pageable costs, is what the reference's callers pass)")
    ap.add_argument("--graph", action="store_true",
                    help="one GPU: compute_rnnt_loss_async captured into a HIP graph once, step = replay + device sync")
    ap.add_argument("--overlap-collective", action="store_true",
                    help="sharded step through the two-phase entry with the all-reduce BESIDE the gradient pass (A/B runs)")
    ap.add_argument("--torch-collective", action="store_true",
                    help="sharded step: torch.sum + torch.distributed.all_reduce instead of compute_rnnt_loss_sharded "
                         "(the library's own ncclAllReduce of [sum, count]) -- A/B runs")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="--gpus N > 1: samples of the whole job, split N ways (default: 1024 for c5 = BASELINE config 5, "
                         "else the workload's own N); must be a multiple of N")
    ap.add_argument("--per-gpu-batch", type=int, default=None,
                    help="--gpus N > 1: the WEAK-scaling form instead -- this many samples on every GPU (global batch = B*N)")
    ap.add_argument("--oversubscribe-gloo", action="store_true",
                    help="dev: the N ranks share the visible device(s) (rank r -> device r %% visible) and talk over gloo; "
                         "exercises the launcher / gather / JSON plumbing on a one-GPU box.  NOT a scaling measurement")
    ap.add_argument("--aux-stream", action="store_true",
                    help="hand the library a second stream (rnnt_set_aux_stream): long lattices (c4) then run the two-half "
                         "schedule -- the lattice kernel of one half of the batch beside the streaming kernels of the other")
    ap.add_argument("--in-place", action="store_true",
                    help="gradients == activations (rnnt.h, IN PLACE): the gradient overwrites the logits; every step restores "
                         "nothing -- after the first step the 'logits' are gradients, the arithmetic and the traffic are the same")
    ap.add_argument("--force-sharded", action="store_true",
                    help="dev: run the multi-GPU step (async entry + RCCL all-reduce) even with one rank")
    ap.add_argument("--no-full-batch", action="store_true",
                    help="--gpus N > 1: skip rank 0's run of the whole global batch on one GPU (multi_gpu.one_gpu_full_batch_ms)")
    ap.add_argument("--no-traffic-pass", action="store_true",
                    help="with --full: do not run the two extra rocprofv3 --pmc passes that measure `roofline.traffic` for this run "
                         "(one GPU only; the figure of the newest committed profiles/r*_traffic.json is reported instead)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the headline's last timed step computed (costs, gradients: a fixed "
                         "sample when larger than %d elements) to DIR/<name>.npy, float32 / float64, rank 0" % DUMP_SAMPLE)
    ap.add_argument("--no-verify", action="store_true",
                    help="with --full: skip the parity check of the timed batch (two samples against the fp64 oracle, outside the "
                         "timed region; its result is the JSON line's `check` object)")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:
        # a plain run: nothing but the headline's own steps (the --no-* options are what --full can be trimmed with)
        args.no_cpu_baseline = args.no_verify = args.no_traffic_pass = args.no_extra = True
    plain_line = not (args.override or args.varlen or args.packed or args.graph or args.aux_stream or args.pinned_costs
                      or args.force_sharded or args.in_place)
    want_extra = args.gpus == 1 and not args.no_extra and (args.extra or (args.workload is None and plain_line))
    if args.workload is None:
        args.workload = "c3" if args.gpus == 1 else "c5"

    if not torch.cuda.is_available():
        print("bench.py needs an MI355X: the HIP path has no CPU fallback", file=sys.stderr)
        raise SystemExit(2)
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and not args.oversubscribe_gloo:
        print("bench.py: --gpus %d asked for, %d device(s) visible -- refusing to run on fewer GPUs than requested"
              % (args.gpus, ndev), file=sys.stderr)
        raise SystemExit(2)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: become the launcher of N ranks (one per GPU, RCCL), rendezvous on
        # 127.0.0.1 (the container's hostname may not resolve)
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        # the host driver only supports dmabuf IPC: without this RCCL's peer setup fails (hipIpcGetMemHandle)
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        raise SystemExit(subprocess.call(cmd, env=env, stdout=real_stdout))      # (rank 0 of the job writes the JSON line)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world), file=sys.stderr)
        raise SystemExit(2)
    gloo = args.oversubscribe_gloo and world > 1
    dev_index = local_rank % ndev if gloo else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    sharded = world > 1 or args.force_sharded
    if sharded:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        elif gloo:
            dist.init_process_group("gloo")                   # ranks may share a device: RCCL would refuse
        else:
            dist.init_process_group("nccl", device_id=dev)   # "nccl" is RCCL on ROCm
    # gloo moves CUDA tensors for all_reduce / broadcast only: the bookkeeping collectives go through the host there
    meta_dev = torch.device("cpu") if gloo else dev

    def barrier():
        torch.cuda.synchronize(dev)
        dist.barrier()

    from warprnnt_pytorch import _lib, warp_rnnt
    lib = _lib.lib()
    aux_stream = None
    if args.aux_stream:
        aux_stream = torch.cuda.Stream(dev)                       # the caller's stream: the library creates none
        lib.rnnt_set_aux_stream(aux_stream.cuda_stream)

    def gather_ints(v):
        mine = torch.tensor([int(v)], dtype=torch.int64, device=meta_dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        return [int(t[0]) for t in every]

    def run_workload(name, steps, warmup, with_cpu, dump_dir=None):
        w = dict(WORKLOADS[name])
        for kv in filter(None, args.override.split(",")):
            k, v = kv.split("=")
            w[k] = v if k == "dtype" else int(v)
            w["published_ms"] = None
        # sharded runs: the GLOBAL batch is the workload (config 5: 1024 samples at every N), a rank holds 1/world of it;
        # --per-gpu-batch: the weak form; one forced rank (--force-sharded): the workload's own N
        scaling, global_batch = "weak", w["N"] * world
        if world > 1 and args.per_gpu_batch:
            w["N"] = args.per_gpu_batch
            global_batch = w["N"] * world
        elif world > 1:
            global_batch = args.global_batch or SHARDED_GLOBAL_BATCH.get(name, w["N"])
            if global_batch % world:
                raise SystemExit("bench.py: global batch %d is not a multiple of %d ranks" % (global_batch, world))
            w["N"] = global_batch // world
            scaling = "strong"
        # the whole global batch on ONE GPU (rank 0, before anything else is resident; the other ranks wait): what the
        # sharded step's time is read against
        full_ms = None
        if world > 1 and scaling == "strong" and not args.no_full_batch:
            if rank == 0:
              fa = fl = ftl = fll = fg = fws = fc = None           # the failing path must drop them too (an OOM here kept ~34 GB alive)
              try:
                  wf = dict(w, N=global_batch)
                  fa, fl, ftl, fll = make_inputs(wf, dev, 999)
                  fg = torch.empty_like(fa)
                  fws = torch.empty(_lib.workspace_bytes(wf["T"], wf["L"] + 1, global_batch, True, ESIZE[w["dtype"]]), dtype=torch.uint8, device=dev)
                  fc = torch.zeros(global_batch, dtype=torch.float32, device=dev)
                  fopt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream,
                                          blank_label=0, maxT=wf["T"], maxU=wf["L"] + 1, batch_first=True)
                  fargv = (fa.data_ptr(), fg.data_ptr(), fl.data_ptr(), fll.data_ptr(), ftl.data_ptr(), wf["A"], global_batch,
                           fc.data_ptr(), None, fws.data_ptr(), fopt, {"fp32": _lib.DT_F32, "bf16": _lib.DT_BF16}[w["dtype"]])
                  for _ in range(2):
                      assert lib.compute_rnnt_loss_async(*fargv) == 0
                      torch.cuda.synchronize(dev)
                  f0 = time.perf_counter()
                  nfull = steps
                  for _ in range(nfull):
                      assert lib.compute_rnnt_loss_async(*fargv) == 0
                      torch.cuda.synchronize(dev)
                  full_ms = (time.perf_counter() - f0) * 1e3 / nfull
              except Exception as exc:                                 # noqa: BLE001 -- the one-GPU base is an extra: without it the line has no speed-up, not no line
                print("bench.py: the whole global batch on one GPU failed (%r); multi_gpu.one_gpu_full_batch_ms is left out" % (exc,), file=sys.stderr)
                full_ms = None
              finally:
                fa = fl = ftl = fll = fg = fws = fc = None
                torch.cuda.empty_cache()
            barrier()
        acts, labels, act_lens, label_lens = make_inputs(w, dev, 1234 + rank)
        N, T, U, A = acts.shape
        if args.varlen:
            g2 = torch.Generator(device=dev); g2.manual_seed(2)
            act_lens = torch.randint(T // 2, T + 1, (N,), generator=g2, device=dev, dtype=torch.int32)
            label_lens = torch.randint((U - 1) // 2, U, (N,), generator=g2, device=dev, dtype=torch.int32)
            act_lens[0], label_lens[0] = T, U - 1
        offs = None
        if args.packed:
            from warprnnt_pytorch.packed import pack_joint, row_offsets
            assert args.varlen and not sharded, "--packed goes with --varlen on one GPU"
            acts_padded = acts
            acts = pack_joint(acts_padded, act_lens, label_lens).contiguous()
            del acts_padded
            torch.cuda.empty_cache()
            offs = row_offsets(act_lens, label_lens)
        grads = acts if args.in_place else torch.empty_like(acts)
        esz = ESIZE[w["dtype"]]
        ws = torch.empty(_lib.workspace_bytes(T, U, N, True, esz), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=stream, blank_label=0, maxT=T,
                               maxU=U, batch_first=True)
        rccl_lib = comm = None
        if args.packed:
            costs = torch.zeros(N, dtype=torch.float32, device=dev)
            code = {"fp32": _lib.DT_F32, "bf16": _lib.DT_BF16}[w["dtype"]]
            argv = (acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lens.data_ptr(), act_lens.data_ptr(),
                    offs.data_ptr(), acts.shape[0], A, N, costs.data_ptr(), None, ws.data_ptr(), opt, code, 0.0)

            def step():
                st = lib.compute_rnnt_loss_packed(*argv)
                assert st == 0, _lib.status_string(st)
                torch.cuda.synchronize(dev)
                lib.rnnt_profile_collect()
                return costs
        elif args.graph and not sharded:
            # the asynchronous entry (device costs) captured ONCE into a HIP graph; a step = one replay + one device sync.
            # For launch-bound problems (c2: four kernels of a few microseconds) the replay replaces four host launches.
            costs = torch.zeros(N, dtype=torch.float32, device=dev)
            code = {"fp32": _lib.DT_F32, "bf16": _lib.DT_BF16}[w["dtype"]]
            cap = torch.cuda.Stream(dev)
            cap.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(cap):
                gopt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=cap.cuda_stream, blank_label=0, maxT=T,
                                        maxU=U, batch_first=True)
                gargv = (acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lens.data_ptr(), act_lens.data_ptr(),
                         A, N, costs.data_ptr(), None, ws.data_ptr(), gopt, code)
                assert lib.compute_rnnt_loss_async(*gargv) == 0            # warm-up outside the capture
                cap.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=cap):
                    st = lib.compute_rnnt_loss_async(*gargv)
                assert st == 0, _lib.status_string(st)
            torch.cuda.current_stream(dev).wait_stream(cap)

            def step():
                graph.replay()
                torch.cuda.synchronize(dev)
                return costs
        elif not sharded:
            # the drop-in C-ABI call: host costs, one stream sync per call
            fn = {"fp32": lib.compute_rnnt_loss, "bf16": lib.compute_rnnt_loss_bf16}[w["dtype"]]
            costs = torch.zeros(N, dtype=torch.float32, pin_memory=args.pinned_costs)
            argv = (acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lens.data_ptr(),
                    act_lens.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(), opt)

            def step():
                st = fn(*argv)
                assert st == 0, _lib.status_string(st)
                return costs
        else:
            # sharded: device costs, one RCCL all-reduce of [sum, count], one sync per step
            costs = torch.zeros(N, dtype=torch.float32, device=dev)
            code = {"fp32": _lib.DT_F32, "bf16": _lib.DT_BF16}[w["dtype"]]
            argv = (acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lens.data_ptr(),
                    act_lens.data_ptr(), A, N, costs.data_ptr(), None, ws.data_ptr(), opt, code)
            fwd_argv = (acts.data_ptr(), labels.data_ptr(), label_lens.data_ptr(), act_lens.data_ptr(), A, N,
                        costs.data_ptr(), ws.data_ptr(), opt, code, 1)
            bwd_argv = (acts.data_ptr(), grads.data_ptr(), None, A, N, ws.data_ptr(), opt, code)
            # the one collective of the data path: an 8-byte all-reduce of the summed loss (RCCL over xGMI).  Every rank
            # holds N samples here, so the sample count of the mean is N * world on the host -- nothing else is
            # written, copied or allocated per step (ShardedRNNTLoss, for ragged shards, reduces [sum, count]).
            packed = torch.zeros(1, dtype=torch.float64, device=dev)

            def reduce_loss(async_op):
                torch.sum(costs, dim=0, keepdim=True, dtype=torch.float64, out=packed)
                return dist.all_reduce(packed, async_op=async_op)

            rccl_lib, comm = (None, None) if (args.torch_collective or args.overlap_collective or gloo) else native_communicator(world, rank, dev)
            pair = torch.zeros(2, dtype=torch.float64, device=dev)       # [summed loss, sample count] of the whole job
            sh_argv = (acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lens.data_ptr(), act_lens.data_ptr(), A, N,
                       costs.data_ptr(), None, pair.data_ptr(), comm, ws.data_ptr(), opt, code)
            collective = ("compute_rnnt_loss_sharded: one ncclAllReduce of [sum, count] (16 B) issued by the library on the compute "
                          "stream" if comm is not None else "torch.sum + torch.distributed.all_reduce of the summed loss (8 B)")
            if comm is not None:
                def step():
                    # the whole sharded step behind the C-ABI: loss + gradients of this rank's shard, the shard's [sum, count],
                    # ONE in-place ncclAllReduce of those 16 bytes over xGMI -- then the one device synchronisation of the step
                    st = lib.compute_rnnt_loss_sharded(*sh_argv)
                    assert st == 0, _lib.status_string(st)
                    torch.cuda.synchronize(dev)
                    lib.rnnt_profile_collect()
                    return pair
            elif args.overlap_collective:
                def step():
                    # two-phase entry: the costs exist after the forward phase, so the collective (16 bytes, RCCL's own
                    # stream) can run BESIDE the gradient pass.  Measured on one rank (`profiles/r02x_*`): the two
                    # cross-stream event waits cost more (+30 us) than a one-rank collective takes, so this is an option
                    # for multi-GPU A/B runs, not the default.
                    st = lib.compute_rnnt_loss_fwd(*fwd_argv)
                    assert st == 0, _lib.status_string(st)
                    work = reduce_loss(True)
                    st = lib.compute_rnnt_loss_bwd(*bwd_argv)
                    assert st == 0, _lib.status_string(st)
                    work.wait()                                  # the compute stream waits for the reduced loss
                    torch.cuda.synchronize(dev)
                    lib.rnnt_profile_collect()
                    return packed
            else:
                def step():
                    st = lib.compute_rnnt_loss_async(*argv)
                    assert st == 0, _lib.status_string(st)
                    reduce_loss(False)
                    torch.cuda.synchronize(dev)
                    lib.rnnt_profile_collect()
                    return packed

        # Sharded runs: the SAME per-GPU workload first WITHOUT the collective (compute_rnnt_loss_async + device sync),
        # on every rank at once -- the single-GPU reference the scaling efficiency of this line is read against
        # (bench.py --gpus 1 times c3, the headline workload, so the driver's 1 -> N curve alone compares two workloads).
        local_ms = None
        if sharded:
            for _ in range(max(warmup, 2)):
                assert lib.compute_rnnt_loss_async(*argv) == 0
                torch.cuda.synchronize(dev)
            barrier()
            l0 = time.perf_counter()
            for _ in range(steps):
                assert lib.compute_rnnt_loss_async(*argv) == 0
                torch.cuda.synchronize(dev)
            local_ms = (time.perf_counter() - l0) * 1e3 / steps
        for _ in range(warmup):
            step()
        lib.rnnt_profile_reset()
        lib.rnnt_profile_enable(1)
        if sharded:
            barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        marks = []
        for _ in range(steps):
            out = step()                          # every form of step() ends with a device synchronisation
            marks.append(time.perf_counter())
        torch.cuda.synchronize(dev)
        if sharded:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        lib.rnnt_profile_enable(0)
        per_step = np.diff(np.array([t0] + marks)) * 1e3
        if dump_dir is not None and rank == 0:
            dump_outputs(dump_dir, costs, grads, out if sharded else None)
        # Small problems only: the same loop once more WITHOUT the per-stage HIP events (five event records per step
        # sit between the kernels; on a 0.08 ms step they are ~10 % of it, on c3 they are not measurable).  Reported
        # next to `value`, which stays the contractual events-on measurement.  A run of its own: --full only.
        plain = None
        if args.full and elapsed * 1e3 / steps < 0.5 and not sharded:
            for _ in range(3):
                step()
            torch.cuda.synchronize(dev)
            p0 = time.perf_counter()
            pm = []
            for _ in range(steps):
                step()
                pm.append(time.perf_counter())
            pp = np.diff(np.array([p0] + pm)) * 1e3
            plain = dict(mean=round(float(pp.mean()), 4), median=round(float(np.median(pp)), 4),
                         p10=round(float(np.percentile(pp, 10)), 4), p90=round(float(np.percentile(pp, 90)), 4),
                         note="the same steps with the per-stage HIP events switched off")
        multi = None
        if sharded:
            mine = torch.tensor([elapsed * 1e3 / steps, local_ms, float(out[0])], dtype=torch.float64, device=meta_dev)
            every = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            per_rank = [float(t[0]) for t in every]
            per_rank_local = [float(t[1]) for t in every]
            reduced = [float(t[2]) for t in every]                     # every rank's copy of the all-reduced loss
            elapsed = max(per_rank) * steps / 1e3                      # MAX over ranks, as the contract asks
            try:
                rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:                                          # noqa: BLE001 -- version query only
                rccl = None
            multi = dict(ranks_seen=dist.get_world_size(), backend=dist.get_backend(), rccl_version=rccl,
                         devices=sorted({int(x) for x in gather_ints(dev_index)}),
                         per_rank_ms=[round(v, 4) for v in per_rank],
                         single_gpu_same_workload_ms=round(max(per_rank_local), 4),
                         per_rank_single_gpu_ms=[round(v, 4) for v in per_rank_local],
                         scaling_efficiency=round(max(per_rank_local) / max(per_rank), 4),
                         reduced_loss_agrees=bool(max(reduced) - min(reduced) <= 1e-9 * max(1.0, abs(reduced[0]))),
                         collective=collective,
                         note="single_gpu_same_workload_ms = the same per-GPU shard through compute_rnnt_loss_async + "
                              "device sync with NO collective, all ranks at once (max over ranks); scaling_efficiency = "
                              "that / value (1.0 = the all-reduce and the barrier are free)")
            if full_ms is not None or (world > 1 and scaling == "strong" and not args.no_full_batch):
                fm = torch.tensor([full_ms if full_ms is not None else 0.0], dtype=torch.float64, device=meta_dev)
                dist.broadcast(fm, src=0)
                full = float(fm[0])
                if full > 0.0:                                      # (0: rank 0's whole-batch run failed and said so on stderr)
                  multi.update(one_gpu_full_batch_ms=round(full, 4), speedup=round(full / max(per_rank), 4),
                             strong_scaling_efficiency=round(full / max(per_rank) / world, 4),
                             strong_note="one_gpu_full_batch_ms = the WHOLE global batch (%d samples) through compute_rnnt_loss_async "
                                         "+ device sync on rank 0's GPU alone; speedup = that / value; "
                                         "strong_scaling_efficiency = speedup / n_gpus" % global_batch)
            if gloo:
                multi["oversubscribed"] = ("%d ranks on %d device(s) over gloo: launcher / gather / JSON plumbing only, "
                                           "the times are NOT a scaling measurement" % (world, ndev))
        ms_step = elapsed * 1e3 / steps
        stage = (C.c_double * 5)()
        calls = lib.rnnt_profile_read(stage, 5)
        stage_ms = [stage[i] / calls for i in range(5)] if calls else None
        valid_rows = int((act_lens.long() * (label_lens.long() + 1)).sum().item()) if args.varlen else None
        ab = algorithmic_bytes(w, valid_rows, args.packed)
        res = dict(workload=name, ms_per_step=ms_step, stage_ms=stage_ms, bytes=ab, w=w, scaling=scaling, global_batch=global_batch,
                   step_ms=dict(median=round(float(np.median(per_step)), 4), p10=round(float(np.percentile(per_step, 10)), 4),
                                p90=round(float(np.percentile(per_step, 90)), 4), n=int(per_step.size),
                                note="per-step wall clock on rank 0 (each step ends in a device sync)"),
                   plain_step_ms=plain, multi=multi,
                   loss_sum=float(out.sum()) if not sharded else float(out[0]))
        if rank == 0 and not args.no_verify and not args.packed:
            picked = None
            if args.in_place:
                # the timed steps have long turned the logits into gradients of gradients: one more step on fresh logits (same
                # seed), outside the timed region, is what the check judges
                fresh = make_inputs(w, dev, 1234 + rank)[0]
                picked = fresh[sorted({0, N - 1})].clone()
                acts.copy_(fresh)
                del fresh
                step()
                torch.cuda.synchronize(dev)
            res["verify"] = verify_batch(w, acts, labels, act_lens, label_lens, grads, costs, picked)
        if with_cpu and rank == 0 and not args.packed:
            res["cpu"] = cpu_baseline(w, acts, labels, act_lens, label_lens, args.cpu_samples)
        if comm is not None:
            torch.cuda.synchronize(dev)
            lib.rnnt_sharded_release(comm)
            rccl_lib.ncclCommDestroy(comm)
        del acts, grads, ws
        torch.cuda.empty_cache()
        return res

    r = run_workload(args.workload, args.steps, args.warmup, with_cpu=(not sharded and not args.no_cpu_baseline),
                     dump_dir=args.dump_outputs)
    w, ab = r["w"], r["bytes"]
    ms = r["ms_per_step"]
    U = w["L"] + 1
    out = {
        "metric": "ms/batch RNN-T loss+grad (N,T,U,A); achieved HBM GB/s vs peak",
        "value": round(ms, 4), "unit": "ms/batch", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms, 4), "higher_is_better": False,
        "scaling": r["scaling"], "vs_baseline": (round(ms / w["published_ms"], 5) if w["published_ms"] else None),
        "dtype": {"fp32": "f32", "bf16": "bf16"}[w["dtype"]], "data": "synthetic",
        "config": {"workload": "%s: N=%d/GPU T=%d U=%d(L=%d) A=%d %s, loss+grad via compute_rnnt_loss%s"
                               % (args.workload, w["N"], w["T"], U, w["L"], w["A"], w["dtype"],
                                  (", VARIABLE lengths T_b~U[T/2,T] L_b~U[L/2,L]" if args.varlen else "")
                                  + (", PACKED layout (compute_rnnt_loss_packed)" if args.packed else "")
                                  + (", host costs in pinned memory" if args.pinned_costs else "")
                                  + (", IN PLACE (gradients == activations)" if args.in_place else "")
                                  + (", compute_rnnt_loss_async replayed from a HIP graph" if args.graph else "")
                                  + (", second stream handed to the library (rnnt_set_aux_stream: two-half schedule on long lattices)"
                                     if args.aux_stream else "")),
                   "global_batch": r["global_batch"], "per_gpu_batch": w["N"],
                   "parallelism": "batch-sharded x%d, one RCCL all-reduce of the summed loss" % world
                   if sharded else "single GPU"},
        "check": dict({"loss_sum": r["loss_sum"], "note": "summed loss of the last step (all ranks when sharded)"},
                      **(r.get("verify") or {})),
        "samples_per_s": round(r["global_batch"] / (ms * 1e-3), 1),
        "step_ms": r["step_ms"],
        "plain_step_ms": r["plain_step_ms"],
        "path_roofline": {"bound": "hbm", "achieved": round(ab["path"] / (ms * 1e-3) / 1e9, 1),
                          "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": round(ab["path"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                          "bytes_algo": ab["path"], "note": "3*E*s + 48*R over the whole step (wall clock, "
                          "incl. launches, costs D2H and sync); aggregate over %d GPU(s) = x%d" % (world, world)},
    }
    if r["stage_ms"]:
        sm = r["stage_ms"]
        gk = sm[3]
        traffic = None
        traffic_file = None
        traffic_source = None
        if not sharded and not args.no_traffic_pass and not args.packed and not args.graph:
            tail = ["--workload", args.workload] + (["--aux-stream"] if args.aux_stream else [])
            if args.override:
                tail += ["--override", args.override]
            if args.varlen:
                tail += ["--varlen"]
            traffic = measure_traffic(tail)
            if traffic is not None:
                traffic_source = ("measured for this run: two extra passes of the same workload under rocprofv3 --pmc FETCH_SIZE / "
                                  "--pmc WRITE_SIZE with --kernel-trace (3 steps each, outside the timed region), 2 x FETCH + WRITE")
        if traffic is None:
            try:   # fallback: the committed rocprofv3 passes of the newest round
                import glob
                traffic_file = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))[-1]
                tj = json.load(open(traffic_file))
                if not args.override and not args.varlen:
                    traffic = tj[args.workload]["grad_flat_kernel"]["traffic_bytes"]
                    traffic_source = "profiles/%s (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; not measured in this run)" \
                                     % os.path.basename(traffic_file)
            except (OSError, KeyError, ValueError, IndexError):
                pass
        out["roofline"] = {"bound": "hbm", "kernel": "grad_flat_kernel (second read of the logits + dense gradient write-back)",
                           "achieved": round(ab["grad_kernel"] / (gk * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(ab["grad_kernel"] / (gk * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "traffic": traffic, "bytes_algo": ab["grad_kernel"], "avg_ms": round(gk, 4),
                           "traffic_source": traffic_source}
        out["stage_ms"] = {"row_stats": round(sm[0], 4), "lattice": round(sm[1], 4), "coef": round(sm[2], 4),
                           "grad": round(sm[3], 4), "enqueue_span": round(sm[4], 4)}
        out["stats_roofline"] = {"achieved": round(ab["stats_kernel"] / (sm[0] * 1e-3) / 1e9, 1),
                                 "frac": round(ab["stats_kernel"] / (sm[0] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                 "unit": "GB/s"}
    if r.get("multi"):
        out["multi_gpu"] = r["multi"]
    if "cpu" in r:
        out["cpu_baseline"] = r["cpu"]
    if want_extra and not sharded:
        # The rest of BASELINE.json's configurations and the additive joint, in the SAME driver-run line, each with its own
        # check against the oracle on two samples of ITS timed batch: c3 is the configuration the metric is quoted on, but
        # nobody should have to take the other numbers on the builder's word.  Protocol as the headline's (warmed, per-step
        # device sync, HIP-event stage times; the reference's own harness: tests/test_time.cu:89-128).
        extra = {}
        esteps, ewarm = args.steps, max(2, min(args.warmup, 5))
        for key, name in OTHER_WORKLOADS.items():
            t_e = time.perf_counter()
            try:
                e = run_workload(name, esteps, ewarm, with_cpu=False)
            except Exception as exc:                                   # noqa: BLE001 -- an extra workload must never cost the headline its line
                extra[key] = {"error": repr(exc)[:400], "check": {"passed": False}}
                torch.cuda.empty_cache()
                continue
            eb, ew, ems = e["bytes"], e["w"], e["ms_per_step"]
            sm = e["stage_ms"]
            rec = {"workload": "%s: N=%d T=%d U=%d(L=%d) A=%d %s, loss+grad via compute_rnnt_loss%s"
                               % (name, ew["N"], ew["T"], ew["L"] + 1, ew["L"], ew["A"], ew["dtype"], "" if ew["dtype"] == "fp32" else "_" + ew["dtype"]),
                   "ms_per_step": round(ems, 4), "step_ms": e["step_ms"], "plain_step_ms": e["plain_step_ms"],
                   "stage_ms": ({"row_stats": round(sm[0], 4), "lattice": round(sm[1], 4), "coef": round(sm[2], 4), "grad": round(sm[3], 4)}
                                if sm else None),
                   "path_frac": round(eb["path"] / (ems * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "bytes_algo": eb["path"],
                   "roofline": ({"bound": "hbm", "kernel": "grad_flat_kernel", "achieved": round(eb["grad_kernel"] / (sm[3] * 1e-3) / 1e9, 1),
                                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(eb["grad_kernel"] / (sm[3] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                 "bytes_algo": eb["grad_kernel"], "avg_ms": round(sm[3], 4)} if sm else None),
                   "samples_per_s": round(ew["N"] / (ems * 1e-3), 1),
                   "vs_published_1080ti": (round(ems / ew["published_ms"], 5) if ew["published_ms"] else None),
                   "check": dict({"loss_sum": e["loss_sum"]}, **(e.get("verify") or {})),
                   "wall_s": round(time.perf_counter() - t_e, 2)}
            # HBM traffic of its gradient kernel: the committed rocprofv3 --pmc passes of the newest profile set (the headline's is
            # measured for THIS run; running two more profiler passes per extra workload would triple the line's wall clock)
            try:
                import glob
                tfile = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))[-1]
                tb = json.load(open(tfile))[name]["grad_flat_kernel"]["traffic_bytes"]
                if rec["roofline"] is not None:
                    rec["roofline"]["traffic"] = tb
                    rec["roofline"]["traffic_source"] = "profiles/%s (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; not measured in this run)" % os.path.basename(tfile)
            except (OSError, KeyError, ValueError, IndexError):
                pass
            extra[key] = rec
        for key in ADD_WORKLOADS:
            t_e = time.perf_counter()
            try:
                rec = run_add_workload(lib, dev, key, esteps, ewarm, verify=not args.no_verify)
            except Exception as exc:                                   # noqa: BLE001
                extra[key] = {"error": repr(exc)[:400], "check": {"passed": False}}
                torch.cuda.empty_cache()
                continue
            rec["wall_s"] = round(time.perf_counter() - t_e, 2)
            extra[key] = rec
        for key in MODULE_WORKLOADS:
            t_e = time.perf_counter()
            try:
                rec = run_rnntloss_workload(dev, key, esteps, ewarm, verify=not args.no_verify)
            except Exception as exc:                                   # noqa: BLE001
                extra[key] = {"error": repr(exc)[:400], "check": {"passed": False}}
                torch.cuda.empty_cache()
                continue
            rec["wall_s"] = round(time.perf_counter() - t_e, 2)
            extra[key] = rec
        out["other_workloads"] = extra
        out["other_workloads_all_checks_passed"] = bool(all((v.get("check") or {}).get("passed", args.no_verify) for v in extra.values()))
    elif r.get("multi") and r["multi"].get("one_gpu_full_batch_ms") is not None and args.workload == "c5":
        # the N > 1 line names the one-GPU base of its strong scaling with the SAME key the one-GPU line uses
        out["other_workloads"] = {"c5_full_1024_on_one_gpu": {
            "workload": "c5_full: N=%d T=200 U=41(L=40) A=1024 bf16 on rank 0's GPU alone (compute_rnnt_loss_async + device sync)" % r["global_batch"],
            "ms_per_step": r["multi"]["one_gpu_full_batch_ms"]}}
    if sharded:
        dist.destroy_process_group()
    # RCCL prints its version banner through C stdio: flush it (to stderr, see the top of main) before stdout comes back
    try:
        C.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    os.close(real_stdout)
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
