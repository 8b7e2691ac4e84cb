"""No GPU: the TDT alignment's fp64 reference (tests/tdt_align_ref.py) against brute-force path enumeration, closed forms and
the loss's reference, and libwarprnnt_tdt_align.so's C-ABI, Python table and code objects against include/rnnt_tdt_align.h and
tests/tdt_align_forms.py."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import tdt_align_forms as F
from tests import tdt_align_ref as R
from tests import tdt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_tdt_align.so", "rnnt_tdt_align.h"
SETS = [(0, 1, 2, 3, 4), (0, 2, 4), (1, 2), (1,)]                  # (tests/test_tdt_cpu.py's)
OLDER = ("libwarprnnt.so", "libwarprnnt_pruned.so", "libwarprnnt_tdt.so", "libwarprnnt_hat.so", "libwarprnnt_mblank.so")
PLANTS = range(4)                                                  # the seeds tests/test_gpu_tdt_align.py plants


def assert_labelling(frames, durs, T, L, durations):
    """Feasible and monotone: frames in [0, T - 1], durations of the set, frames[u] + durs[u] <= frames[u + 1], the last
    label's edge ends inside the grid; -1 behind L."""
    assert (frames[L:] == -1).all() and (durs[L:] == -1).all(), (frames, durs, L)
    f, d = frames[:L].astype(int), durs[:L].astype(int)
    assert ((f >= 0) & (f <= T - 1)).all() and all(v in durations for v in d), (f, d)
    assert (f[:-1] + d[:-1] <= f[1:]).all() and (f + d <= T - 1).all(), (f, d)


@pytest.mark.parametrize("seed", range(50))
def test_best_path_equals_brute_force(seed):
    rng = np.random.default_rng(2000 + seed)
    durs = SETS[seed % len(SETS)]
    N = 3
    T, U, A = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(2, 6))
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    ll[1] = 0                                                     # L_b = 0
    blank = A - 1 if seed % 2 else 0
    sigma = 0.05 if seed % 3 == 0 else 0.0
    x = rng.standard_normal((N, T, U, A + len(durs))) * 1.5
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    score, frames, dd = R.best_path(x, labels, tl, ll, durs, blank, sigma)
    again = R.rescore(x, labels, tl, ll, durs, blank, sigma, frames, dd)
    for b, (want, _) in enumerate(R.brute(x, labels, tl, ll, durs, blank, sigma)):
        if not np.isfinite(want):
            assert score[b] == -np.inf and (frames[b] == -1).all() and (dd[b] == -1).all()
            continue
        assert abs(score[b] - want) <= 1e-12 * max(1.0, abs(want)), (b, score[b], want)
        assert abs(again[b] - score[b]) <= 1e-12 * max(1.0, abs(want)), (b, again[b], score[b])
        assert_labelling(frames[b], dd[b], int(tl[b]), int(ll[b]), durs)


def test_rescore_refuses_an_infeasible_labelling():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 6, 3, 4 + 3))
    labels = np.array([[1, 2]], np.int32)
    score, frames, dd = R.best_path(x, labels, [6], [2], (0, 1, 2))
    for f, d in (([3, 2], [0, 0]), ([0, 5], [0, 1]), ([0, 1], [3, 0]), ([-1, 1], [0, 0])):
        assert R.rescore(x, labels, [6], [2], (0, 1, 2), 0, 0.0, np.array([f]), np.array([d]))[0] == -np.inf
    assert R.rescore(x, labels, [6], [2], (0, 1, 2), 0, 0.0, frames, dd)[0] == pytest.approx(score[0], abs=1e-12)


def test_infeasible_samples_have_no_path():
    """durations [0, 2] with an odd T_b and L_b = 0: only even frames are reachable, the final blank leaves an odd one."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 5, 1, 3 + 2))
    score, frames, dd = R.best_path(x, np.zeros((2, 0), np.int32), [5, 4], [0, 0], (0, 2))
    assert score[0] == -np.inf and np.isfinite(score[1]) and frames.shape == dd.shape == (2, 0)
    x = rng.standard_normal((1, 5, 2, 3 + 2))
    score, frames, dd = R.best_path(x, np.ones((1, 1), np.int32), [5], [0], (0, 2))
    assert score[0] == -np.inf and (frames == -1).all() and (dd == -1).all()


def test_single_duration_closed_form():
    """durations = [1], T_b = L_b + 1: one path -- the labels on the diagonal, then the final blank."""
    rng = np.random.default_rng(8)
    A, L = 6, 4
    T = L + 1
    x = rng.standard_normal((1, T, L + 1, A + 1))
    labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
    for blank, sigma in ((0, 0.0), (A - 1, 0.05)):
        lp = torch.log_softmax(torch.tensor(x[0, :, :, :A]), -1).numpy() - sigma
        want = sum(lp[u, u, labels[0, u]] for u in range(L)) + lp[L, L, blank]
        score, frames, dd = R.best_path(x, labels, [T], [L], (1,), blank, sigma)
        assert abs(score[0] - want) < 1e-12
        assert frames[0].tolist() == list(range(L)) and dd[0].tolist() == [1] * L


@pytest.mark.parametrize("seed", range(6))
def test_score_is_at_most_the_log_likelihood(seed):
    rng = np.random.default_rng(300 + seed)
    durs = SETS[seed % len(SETS)]
    N, T, U, A = 3, 7, 4, 5
    tl, ll = np.array([7, 6, 5], np.int32), np.array([3, 2, 0], np.int32)
    x = rng.standard_normal((N, T, U, A + len(durs))) * 2
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    score, _, _ = R.best_path(x, labels, tl, ll, durs, 0, 0.05)
    cost, _ = tdt_ref.tdt_autograd(x, labels, tl, ll, durs, 0, 0.05)
    assert (score <= -cost + 1e-12).all() and (score >= -cost - 40).all(), (score, cost)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("seed", PLANTS)
def test_planted_paths_are_recovered(seed, dtype):
    """Every planted case tests/test_gpu_tdt_align.py uses, on the logits as each dtype stores them."""
    x, labels, tl, ll, frames, dd = R.planted(seed)
    stored = torch.tensor(x).to(dtype).double().numpy()
    score, f, d = R.best_path(stored, labels, tl, ll, R.PLANT["durations"])
    assert np.isfinite(score).all() and np.array_equal(f, frames) and np.array_equal(d, dd), (f, frames, d, dd)


# ----------------------------------------------------------------------------- the library and its Python table
def test_exports_equal_the_header():
    declared, exported = I.declared(HEADER), I.exports(I.need_lib(LIB))
    assert declared and exported == declared, (sorted(exported), sorted(declared))


def test_older_libraries_do_not_export_the_new_names():
    new = I.declared(HEADER)
    assert new == {"get_workspace_size_tdt_align", "compute_tdt_align"}
    for lib in OLDER:
        assert not (I.exports(I.need_lib(lib)) & new), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import tdt_align
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(tdt_align.EXPORTS, HEADER) == []


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_device_code_has_no_scratch():
    """No scratch, no spilled VGPRs (tools/check_kernel_resources.py) in any of the three code objects."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as res
    import check_lattice_lin_isa as guard
    for unit in F.OBJECTS.values():
        asm = guard.device_asm(None, os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
        assert res.kernels(asm) and res.check(asm) == [], unit


def test_python_refuses_bad_durations_and_cpu_tensors():
    from warprnnt_pytorch.tdt_align import tdt_align
    args = [torch.zeros(1, 2, 2, 5), torch.zeros(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
            torch.tensor([1], dtype=torch.int32)]
    for d in ((), (1, 1), (2, 1), (-1, 1), (0,), (0, 65), tuple(range(9))):
        with pytest.raises(ValueError):
            tdt_align(*args, d)
    with pytest.raises(ValueError) as e:
        tdt_align(*args, (0, 1))
    assert str(e.value) == "the TDT alignment runs on the GPU only: logits are on cpu"


def test_importing_the_package_does_not_load_the_library():
    import subprocess
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\n"
            "assert 'warprnnt_pytorch.tdt_align' not in sys.modules\n"
            "from warprnnt_pytorch import tdt_align\nassert tdt_align._LIB._handle is None\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
