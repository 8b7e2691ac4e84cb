"""-m gpu: the TDT best-path alignment (include/rnnt_tdt_align.h, libwarprnnt_tdt_align.so).

Every case of tests/tdt_align_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules
predict run, stage by stage.  Every finite sample is held to the fp64 reference of tests/tdt_align_ref.py (on the upcast stored
logits) by one rule:
  (a) |score - ref_score| within side_check.COST_TOL[dtype] (rtol = atol): the project's cost bound -- the score is a sum of
      the same stored log-probs as the cost;
  (b) rescore(gpu_frames, gpu_durs) >= ref_score - tol: a wrong back-pointer or traceback lands far below or at -inf, a
      genuine near-tie passes;
  (c) frames non-decreasing, in [0, T_b - 1], and -1 behind L_b (durs alike);
and for fp64 storage frames and durs equal the reference's exactly.  Ragged lengths (one sample with T_b = 1, one with L_b = 0)
and NaN in every padding row (never read) throughout.  Then the 1024-thread launch, a diagonal wider than the block (T_b and
L_b + 1 both above 1024), the wrap of the offset ring, the long lattice, planted paths, the samples without a path and the poisoned rows, the invalid arguments, one graph capture and the Python
entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import tdt_align_forms as F
from tests import tdt_align_ref as R
from tests.gpu_support import (CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, dev, options, place,
                               profiled, stages_seen)
from tests.test_gpu_tdt import _SETS, _SHAPES, _problem

pytestmark = pytest.mark.gpu
UNSET = -7                                               # what frames and durs hold before a call


def _mod():
    from warprnnt_pytorch import tdt_align
    return tdt_align


class Buffers:
    """The device arrays of one call: outputs that start as NaN / UNSET, the workspace, labels and lengths."""

    def __init__(self, x, labels, tl, ll, D, ws=None):
        N, T, U, _ = x.shape
        self.score = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        self.frames = torch.full((N, max(U - 1, 1)), UNSET, dtype=torch.int32, device=DEV)
        self.durs = torch.full((N, max(U - 1, 1)), UNSET, dtype=torch.int32, device=DEV)
        self.ws = ws if ws is not None else torch.empty(_mod().workspace_bytes(T, U, N, D, CODE[NAME[x.dtype]]),
                                                        dtype=torch.uint8, device=DEV)
        self.lab, self.tl, self.ll = dev(labels if labels.size else np.zeros((N, 1), np.int32), tl, ll)

    def results(self, U):
        return self.score.cpu().numpy(), self.frames.cpu().numpy()[:, :U - 1], self.durs.cpu().numpy()[:, :U - 1]


def enqueue(x, buf, durations, blank=0, sigma=0.0, stream=None):
    N, T, U, W = x.shape
    D = len(durations)
    dur = (C.c_int * max(D, 1))(*durations)
    return _mod().lib().compute_tdt_align(x.data_ptr(), dur, D, sigma, buf.lab.data_ptr(), buf.ll.data_ptr(),
                                          buf.tl.data_ptr(), W - D, N, buf.score.data_ptr(), buf.frames.data_ptr(),
                                          buf.durs.data_ptr(), buf.ws.data_ptr(), options(T, U, blank, stream),
                                          CODE[NAME[x.dtype]])


def call(x, labels, tl, ll, durations, blank=0, sigma=0.0, ws=None):
    """One C-ABI call on the device tensor x -> (status, score, frames, durs).  ws: the caller's workspace."""
    buf = Buffers(x, labels, tl, ll, len(durations), ws)
    st = enqueue(x, buf, durations, blank, sigma)
    torch.cuda.synchronize()
    return (st,) + buf.results(x.shape[2])


def reference(x, labels, tl, ll, durations, blank=0, sigma=0.0):
    """The fp64 reference on the stored logits, upcast (NaN padding rows, never read, as zeros)."""
    xr = torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()
    return xr, R.best_path(xr, labels, tl, ll, durations, blank, sigma)


def check(dtype, xr, labels, tl, ll, durations, blank, sigma, got, ref, what="", samples=None):
    """Rules (a) - (c) of the module docstring for every sample of `samples` (default: all), each of which must be finite in
    the reference; fp64 storage: the labelling itself."""
    score, frames, durs = got
    rs, rf, rd = ref
    tol = COST_TOL[dtype]
    samples = range(len(rs)) if samples is None else samples
    again = R.rescore(xr, labels, tl, ll, durations, blank, sigma, frames, durs)
    for b in samples:
        T, L = int(tl[b]), int(ll[b])
        assert np.isfinite(rs[b]), (what, b, "the reference has no path")
        bound = tol + tol * abs(rs[b])
        print(what, "sample %d: score %.9g ref %.9g (|d| = %.3e, bound %.3e) rescored %.9g" %
              (b, score[b], rs[b], abs(score[b] - rs[b]), bound, again[b]))
        assert abs(score[b] - rs[b]) <= bound, (what, b, score[b], rs[b])                                  # (a)
        assert again[b] >= rs[b] - bound, (what, b, again[b], rs[b], frames[b], rf[b], durs[b], rd[b])     # (b)
        f, d = frames[b, :L], durs[b, :L]                                                                  # (c)
        assert (frames[b, L:] == -1).all() and (durs[b, L:] == -1).all(), (what, b, frames[b], durs[b])
        assert ((f >= 0) & (f <= T - 1)).all() and (np.diff(f) >= 0).all(), (what, b, f)
        assert all(int(v) in durations for v in d) and (f[:-1] + d[:-1] <= f[1:]).all(), (what, b, f, d)
        if dtype == "f64":
            assert np.array_equal(frames[b], rf[b]) and np.array_equal(durs[b], rd[b]), (what, b, frames[b], rf[b], durs[b], rd[b])


def run_and_check(name, dtype, N, T, U, A, durs, blank=0, sigma=0.0, lengths=None, rng=None, scale=2.0, need_labels=True):
    x, labels, tl, ll, _ = _problem(name, dtype, N, T, U, A, durs, rng=rng, lengths=lengths, scale=scale)
    st, *got = call(x.to(DEV), labels, tl, ll, durs, blank, sigma)
    assert st == 0
    xr, ref = reference(x, labels, tl, ll, durs, blank, sigma)
    fin = [b for b in range(N) if np.isfinite(ref[0][b])]
    assert not need_labels or any(ll[b] > 0 for b in fin), (name, ref[0], ll)
    for b in set(range(N)) - set(fin):                              # (sets without 0 need T_b > L_b: no path otherwise)
        assert got[0][b] == -np.inf and (got[1][b] == -1).all() and (got[2][b] == -1).all(), (name, b, got)
    check(dtype, xr, labels, tl, ll, durs, blank, sigma, got, ref, name, fin)


# ----------------------------------------------------------------------------- every form of tests/tdt_align_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_tdt_align_form(name):
    case = F.CASES[name]
    N, T, U, A, durs, dtype = case["N"], case["T"], case["U"], case["A"], case["durations"], case["dtype"]
    x, labels, tl, ll, _ = _problem(name, dtype, N, T, U, A, durs)
    xv = place(x.to(DEV), case.get("off", 0), x.dtype)
    (st, *got), names = profiled(lambda: call(xv, labels, tl, ll, durs))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, G.cus()))
    xr, ref = reference(x, labels, tl, ll, durs)
    fin = [b for b in range(N) if np.isfinite(ref[0][b])]
    assert any(ll[b] > 0 for b in fin), (name, ref[0], ll)
    for b in set(range(N)) - set(fin):
        assert got[0][b] == -np.inf and (got[1][b] == -1).all() and (got[2][b] == -1).all(), (name, b, got)
    check(dtype, xr, labels, tl, ll, durs, 0, 0.0, got, ref, name, fin)


def test_every_tdt_align_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- parity against the fp64 reference
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("shape", range(len(_SHAPES)))
def test_parity(dtype, shape):
    N, T, U, A, durs = _SHAPES[shape]
    run_and_check("apar_%s_%d" % (dtype, shape), dtype, N, T, U, A, durs, blank=A - 1 if shape % 2 else 0,
                  sigma=0.05 if shape % 3 == 1 else 0.0, need_labels=U > 1)


@pytest.mark.parametrize("durs", _SETS)
def test_parity_duration_sets(durs):
    """(T_b is odd for some samples: under (0, 2, 4) those have no path and must come back as -inf and -1s.)"""
    for blank, sigma in ((0, 0.0), (32, 0.05)):
        run_and_check("asets_%s" % (durs,), "f32", 4, 11, 6, 33, durs, blank=blank, sigma=sigma, need_labels=False)


def test_widest_launch():
    """maxU = 1100 launches the full 1024-thread, 16-wave block.  (T_b <= 4 keeps every diagonal at 4 cells or fewer: the
    rounds of a diagonal wider than the block are test_diagonal_wider_than_the_block's.)"""
    rng = np.random.default_rng(21)
    lengths = (np.array([4, 3], np.int32), np.array([1099, 1050], np.int32))
    run_and_check("wide", "f32", 2, 4, 1100, 2, (0, 1, 2), blank=1, lengths=lengths, rng=rng)


def _two_rounds(dtype):
    """T_b = L_b + 1 = 1040: a diagonal holds min(T_b, L_b + 1) cells at the most, so the diagonals 1024 .. 1054 take a
    second round of the 1024-thread block, for the cells (t, u) with u - max(0, t + u - (T_b - 1)) >= 1024 -- the corner
    t <= 15, u >= 1024, which a random best path never visits.  So the logits steer it there, with +3 on the token and the
    duration of every edge of one path: blanks of duration 1 to frame 8, every label there with duration 0, blanks of
    duration 1 to the end.  It runs through the cells (8, 1024 .. 1039) of the second round."""
    N, T, U, A, durs, at = 1, 1040, 1040, 2, (0, 1), 8
    tl, ll = np.array([T], np.int32), np.array([U - 1], np.int32)
    x, labels, tl, ll, _ = _problem("arounds_" + dtype, dtype, N, T, U, A, durs, rng=np.random.default_rng(23),
                                    lengths=(tl, ll), scale=1.0)
    x[0, :at, 0, A - 1] += 3.0
    x[0, :at, 0, A + 1] += 3.0
    x[0, at, np.arange(U - 1), torch.tensor(labels[0], dtype=torch.long)] += 3.0
    x[0, at, :U - 1, A] += 3.0
    x[0, at:, U - 1, A - 1] += 3.0
    x[0, at:, U - 1, A + 1] += 3.0
    xr, ref = reference(x, labels, tl, ll, durs, A - 1)
    return x, labels, tl, ll, durs, xr, ref


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_diagonal_wider_than_the_block(dtype):
    """T_b = L_b + 1 = 1040 > 1024: the strided loop over a diagonal's cells makes a second round, and the best path runs
    through cells computed in it (asserted on the reference's path)."""
    x, labels, tl, ll, durs, xr, ref = _two_rounds(dtype)
    T, L = int(tl[0]), int(ll[0])
    u = np.arange(L)
    t = ref[1][0].astype(np.int64)                                  # the source node (t, u) of label u's edge is on the path
    second = u - np.maximum(0, t + u - (T - 1)) >= 1024
    print("cells of the best path computed in the second round:", int(second.sum()))
    assert second.sum() >= 8, (t[1020:], second.sum())
    st, *got = call(x.to(DEV), labels, tl, ll, durs, blank=1)
    assert st == 0
    check(dtype, xr, labels, tl, ll, durs, 1, 0.0, got, ref, "rounds_" + dtype)


def test_offset_ring_wraps():
    """More than 128 diagonals with d_max = 64: predecessors 65 diagonals back, the ring of offsets in its second lap."""
    rng = np.random.default_rng(22)
    lengths = (np.array([200, 150], np.int32), np.array([2, 1], np.int32))
    run_and_check("ring", "f32", 2, 200, 3, 4, (1, 64), lengths=lengths, rng=rng)


@functools.lru_cache(maxsize=None)
def _long(dtype):
    N, T, U, A = 2, 1500, 301, 3
    durs = (0, 1, 2, 3, 4)
    tl, ll = np.array([T, 1100], np.int32), np.array([U - 1, 250], np.int32)
    x, labels, tl, ll, _ = _problem("along_" + dtype, dtype, N, T, U, A, durs, rng=np.random.default_rng(7), lengths=(tl, ll),
                                    scale=1.0)
    xr, ref = reference(x, labels, tl, ll, durs, A - 1)
    return x, labels, tl, ll, durs, xr, ref


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_long_lattice(dtype):
    """T = 1500, U = 301: 1800 anti-diagonals -- the precision of the values relative to the per-diagonal offsets."""
    x, labels, tl, ll, durs, xr, ref = _long(dtype)
    st, *got = call(x.to(DEV), labels, tl, ll, durs, blank=2)
    assert st == 0 and np.isfinite(ref[0]).all()
    check(dtype, xr, labels, tl, ll, durs, 2, 0.0, got, ref, "long_" + dtype)


# ----------------------------------------------------------------------------- planted paths
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("seed", range(4))
def test_planted_paths(seed, dtype):
    """+12 on the token and duration logits of a random path per sample: frames and durs are the plant's, exactly
    (tests/test_tdt_align_cpu.py shows that the reference recovers each plant in each dtype)."""
    x, labels, tl, ll, frames, durs = R.planted(seed)
    st, score, f, d = call(torch.tensor(x).to(TORCH[dtype]).to(DEV), labels, tl, ll, R.PLANT["durations"])
    assert st == 0 and np.isfinite(score).all()
    assert np.array_equal(f, frames) and np.array_equal(d, durs), (f, frames, d, durs)


# ----------------------------------------------------------------------------- edge cases
def test_no_path_poison_and_bad_lengths_stay_isolated():
    N, T, U, A = 8, 5, 3, 6
    durs = (0, 2)
    rng = np.random.default_rng(5)
    # odd samples are the odd ones out, each next to a healthy even one.  1: L_b = 0 and odd T_b -- only even frames are
    # reachable, the final blank needs T_b - 2 even: no path; 3: a NaN inside the lattice; 5: an all -inf token part;
    # 7: T_b > maxT
    tl = np.array([4, 3, 4, 4, 4, 4, 4, T + 1], np.int32)
    ll = np.array([2, 0, 1, 2, 2, 2, 0, 1], np.int32)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    x = torch.tensor(rng.standard_normal((N, T, U, A + len(durs))) * 2.0, dtype=torch.float32)
    for b in range(N):
        x[b, min(int(tl[b]), T):] = float("nan")
        x[b, :, int(ll[b]) + 1:] = float("nan")
    x[3, 1, 0, 3] = float("nan")
    x[5, 0, 1, :A] = -float("inf")
    x[7] = torch.nan_to_num(x[7])
    st, score, f, d = call(x.to(DEV), labels, tl, ll, durs)
    assert st == 0
    assert score[1] == -np.inf and np.isnan(score[3]) and np.isnan(score[5]) and np.isnan(score[7]), score
    for b in (1, 3, 5, 7):
        assert (f[b] == -1).all() and (d[b] == -1).all(), (b, f[b], d[b])
    healthy = [0, 2, 4, 6]
    tl_ok = np.where(np.arange(N) == 7, T, tl)
    xr, ref = reference(torch.nan_to_num(x, neginf=0.0), labels, tl_ok, ll, durs)
    check("f32", xr, labels, tl_ok, ll, durs, 0, 0.0, (score, f, d), ref, "isolated", healthy)


def test_invalid_arguments_launch_nothing():
    N, T, U, A = 2, 4, 3, 5
    x, labels, tl, ll, _ = _problem("ainv", "f32", N, T, U, A, (0, 1, 2))
    xd = x.to(DEV)

    def refused(x, labels, tl, ll, durs, blank=0):
        buf = Buffers(x, labels, tl, ll, max(min(len(durs), 8), 1))
        st = enqueue(x, buf, durs, blank)
        torch.cuda.synchronize()
        score, f, d = buf.results(max(x.shape[2], 2))
        assert st == 2 and np.isnan(score).all() and (f == UNSET).all() and (d == UNSET).all(), (durs, blank, st)
    for durs in ((), (1, 1), (2, 1), (-1, 1), (0,), (0, 65), tuple(range(9))):
        refused(xd, labels, tl, ll, durs)
    refused(xd, labels, tl, ll, (0, 1, 2), blank=A)
    xb = torch.zeros((1, 1, 4097, 3), device=DEV)
    refused(xb, np.zeros((1, 4096), np.int32), np.array([1], np.int32), np.array([0], np.int32), (1,))


def test_graph_capture_and_replay():
    """The call is enqueue only: recorded once on a side stream (one chain), replayed on fresh inputs."""
    N, T, U, A = 3, 9, 5, 33
    durs = (0, 1, 2, 4)
    x0, labels, tl, ll, _ = _problem("acap0", "f32", N, T, U, A, durs)
    x1, labels1, _, _, _ = _problem("acap1", "f32", N, T, U, A, durs, lengths=(tl, ll))
    static = x0.to(DEV)
    buf = Buffers(static, labels, tl, ll, len(durs))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up outside capture (loads the code object)
        assert enqueue(static, buf, durs, blank=A - 1) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert enqueue(static, buf, durs, blank=A - 1) == 0
    static.copy_(x1)
    buf.lab.copy_(torch.tensor(labels1))
    buf.score.fill_(float("nan")); buf.frames.fill_(UNSET); buf.durs.fill_(UNSET)
    graph.replay()
    torch.cuda.synchronize()
    got = buf.results(U)
    st, *eager = call(x1.to(DEV), labels1, tl, ll, durs, blank=A - 1)
    assert st == 0
    for g, e in zip(got, eager):
        assert np.array_equal(g, e), (g, e)
    xr, ref = reference(x1, labels1, tl, ll, durs, A - 1)
    check("f32", xr, labels1, tl, ll, durs, A - 1, 0.0, got, ref, "replay",
          [b for b in range(N) if np.isfinite(ref[0][b])])


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_python_entry_equals_the_c_abi(dtype):
    from warprnnt_pytorch.tdt_align import tdt_align
    N, T, U, A = 4, 10, 6, 40
    durs = (0, 1, 2, 3)
    x, labels, tl, ll, _ = _problem("apy_" + dtype, dtype, N, T, U, A, durs)
    xd = x.to(DEV).requires_grad_()
    score, frames, dd = tdt_align(xd, *dev(labels, tl, ll), durs, blank=A - 1, sigma=0.05)
    assert score.dtype == torch.float64 and frames.dtype == dd.dtype == torch.int32 and not score.requires_grad
    assert frames.shape == dd.shape == (N, U - 1)
    st, s2, f2, d2 = call(xd.detach(), labels, tl, ll, durs, blank=A - 1, sigma=0.05)
    assert st == 0
    assert np.array_equal(score.cpu().numpy(), s2) and np.array_equal(frames.cpu().numpy(), f2)
    assert np.array_equal(dd.cpu().numpy(), d2)
    # maxU = 1: no labels, empty frames and durs
    x1, l1, tl1, ll1, _ = _problem("apy1_" + dtype, dtype, 2, 5, 1, 7, (1, 2))
    score, frames, dd = tdt_align(x1.to(DEV), torch.zeros((2, 0), dtype=torch.int32, device=DEV), *dev(tl1, ll1), (1, 2))
    _, ref = reference(x1, l1, tl1, ll1, (1, 2))
    assert frames.shape == dd.shape == (2, 0)
    assert np.allclose(score.cpu().numpy(), ref[0], rtol=COST_TOL[dtype], atol=COST_TOL[dtype])


def test_cpu_tensors_are_refused():
    from warprnnt_pytorch.tdt_align import tdt_align
    with pytest.raises(ValueError, match="GPU"):
        tdt_align(torch.zeros(1, 2, 2, 5), torch.zeros(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                  torch.tensor([1], dtype=torch.int32), (0, 1))
