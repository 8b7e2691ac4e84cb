"""No GPU: the fp64 reference of the prune ranges from occupations (tests/ranges_ref.py) against the rule of
include/rnnt_pruned.h (tests/pruned_ref.py) and against its own guarantees; libwarprnnt_ranges.so's C-ABI, export map and code
objects against include/rnnt_ranges.h; the build lists; the argument program under the host sanitizers; and the refusals of
warprnnt_pytorch.ranges that need no device.  A library that is not built is an error here, not a skip."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import pruned_ref
from tests import ranges_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_ranges.so", "rnnt_ranges.h"
NAMES = {"compute_rnnt_prune_ranges_occ", "compute_rnnt_range_coverage"}
OBJECTS = {"f32": "rnnt_ranges.hip", "f64": "rnnt_ranges_f64.hip", "h16": "rnnt_ranges_h16.hip"}


def _lib():
    path = os.path.join(I.LIBDIR, LIB)
    assert os.path.exists(path), "%s is not built" % LIB
    return path


def expected_inventory():
    inv = {}
    for obj, tags in (("f32", ("F32",)), ("f64", ("F64",)), ("h16", ("BF16", "F16"))):
        inv[obj] = {"rnnt::ranges_repair_kernel<0>"}
        for tag in tags:
            for mod in ("true", "false"):
                for kernel in ("ranges_window_kernel", "ranges_coverage_kernel"):
                    inv[obj].add("rnnt::%s<rnnt::%s, %s>" % (kernel, tag, mod))
    return inv


# ----------------------------------------------------------------------------- the reference against the rule it generalises
def _table():
    """About 150 small (T, L, R) with an occupancy of their own: ragged, with near-empty rows, ties and samples whose windows
    cannot hold a path."""
    rng = np.random.default_rng(31)
    out = []
    for k in range(156):
        T, L = int(rng.integers(1, 9)), int(rng.integers(0, 10))
        Rw = int(rng.integers(2, L + 2)) if L >= 1 else 2
        gamma = rng.random((T, L + 1)) ** 3
        if k % 5 == 0:
            gamma = np.round(gamma * 4) / 4                           # ties
        if k % 7 == 0:
            gamma[rng.random(gamma.shape) < 0.4] = 0.0
        out.append((T, L, Rw, gamma))
    return out


def test_step_r_minus_1_is_the_rule_of_the_pruned_library():
    nopath = 0
    for T, L, Rw, gamma in _table():
        got = R.ranges_from_gamma(gamma, T, L, Rw, Rw - 1)
        assert np.array_equal(got, pruned_ref.ranges_rule(gamma, T, L, Rw)), (T, L, Rw)
        smax = max(0, L + 1 - Rw)
        assert (smax > (T - 1) * (Rw - 1)) == (L > T * (Rw - 1))
        nopath += smax > (T - 1) * (Rw - 1)
    assert nopath >= 5 and len(_table()) >= 150


def test_the_guarantees_hold_whenever_the_windows_can_reach():
    """pruned_ref.check_invariants (s_0 = 0, steps in [0, R - 1], s_last = smax, a path through the windows of the regular
    lattice) for every step in [1, R - 1] whenever smax <= (T_b - 1) step.  (R >= 2: with R = 1 no two windows overlap.)"""
    checked = 0
    for T, L, Rw, gamma in _table():
        if Rw > L + 1:
            continue
        for step in sorted({1, Rw - 1, max(1, (Rw - 1) // 2)}):
            smax = max(0, L + 1 - Rw)
            s = R.ranges_from_gamma(gamma, T, L, Rw, step)
            if smax <= (T - 1) * step:
                assert pruned_ref.check_invariants(s, T, L, Rw) == [], (T, L, Rw, step, s)
                assert (np.diff(s) <= step).all()
                checked += 1
            else:
                assert list(s) == [min(t * step, smax) for t in range(T)]
    assert checked >= 150


def test_step_1_guarantees_and_the_modified_lattice():
    """step = 1, the modified type's slope: s_0 = 0, steps in [0, 1], s_last = smax; and where the modified lattice has a path
    at all (S_b <= T_b) one runs through the windows.  R = 1 included."""
    checked = paths = 0
    rng = np.random.default_rng(32)
    for T, L, _, gamma in _table():
        for Rw in sorted({1, 2, int(rng.integers(1, L + 2))}):
            if Rw > L + 1:
                continue
            smax = max(0, L + 1 - Rw)
            s = R.ranges_from_gamma(gamma, T, L, Rw, 1)
            if smax > T - 1:
                assert list(s) == [min(t, smax) for t in range(T)]
                continue
            d = np.diff(s)
            assert s[0] == 0 and s[T - 1] == smax and (d >= 0).all() and (d <= 1).all(), (T, L, Rw, s)
            checked += 1
            if L <= T:
                assert R.modified_path_exists(s, T, L, Rw), (T, L, Rw, s)
                paths += 1
    assert checked >= 150 and paths >= 100


def test_the_reference_reads_nothing_outside_the_rectangle_and_handles_the_edge_cases():
    rng = np.random.default_rng(33)
    B, S, T = 3, 5, 6
    for mod in (False, True):
        px, py = rng.random((B, S, T if mod else T + 1)), rng.random((B, S + 1, T))
        bd = np.array([[0, 0, 5, 6], [0, 0, 2, 1], [0, 0, 0, 4]])
        want = R.prune_ranges(px, py, bd, 3, 2)
        kept = R.coverage(px, py, bd, want, 3)
        qx, qy = px.copy(), py.copy()
        for b, (Sb, Tb) in enumerate(((5, 6), (2, 1), (0, 4))):
            qx[b, Sb:, :] = np.nan
            qx[b, :, Tb:] = np.nan
            qy[b, Sb + 1:, :] = np.nan
            qy[b, :, Tb:] = np.nan
        assert np.array_equal(R.prune_ranges(qx, qy, bd, 3, 2), want)
        assert np.array_equal(R.coverage(qx, qy, bd, want, 3), kept)
        assert (want[1] == 0).all() and (want[2] == 0).all() and (kept[1, 1:] == 0).all() and (kept[2, :4] == 1.0).all()
        assert ((kept >= 0) & (kept <= 1)).all()
    # ties go to the smallest start; all-zero occupations: start 0 (the repair then moves what it must), kept 0
    one, zero = np.ones((1, 7, 4)), np.zeros((1, 7, 4))
    assert list(R.prune_ranges(np.ones((1, 6, 5)), one, None, 3, 2)[0]) == [0, 0, 2, 4]
    assert list(R.prune_ranges(np.zeros((1, 6, 5)), zero, None, 3, 2)[0]) == [0, 0, 2, 4]
    assert (R.coverage(np.zeros((1, 6, 5)), zero, None, np.zeros((1, 4), np.int32), 3) == 0).all()
    # a NaN sum never wins
    g = [1.0, float("nan"), 0.5, 0.25, 0.25]
    assert R.raw_start(g, 2, 4)[0] == 2 and R.raw_start([float("nan")] * 3, 1, 2)[0] == 0
    assert R.raw_start([-1.0, float("nan"), -2.0], 1, 2)[0] == 0 and R.raw_start([float("nan"), float("-inf")], 1, 1)[0] == 1


@pytest.mark.parametrize("seed", R.ADD_SEEDS)
def test_every_seed_of_the_additive_problem_has_clear_windows(seed):
    """tests/test_gpu_ranges.py compares the starts from mi's occupations with prune_ranges(f, g, ...) for these seeds: in
    the fp64 reference best and runner-up window sums differ by at least 1e-3 relative in every frame, far above what two
    lattices in different precisions differ by.  A seed that fails is replaced in ranges_ref.ADD_SEEDS, none is skipped."""
    p = R.additive_problem(seed)
    assert R.ADD_GAP == 1e-3 and p["gap"] >= R.ADD_GAP, (seed, p["gap"])
    # px / py are the joint's lattice: the occupations of the reference lattice over them give the same starts
    from tests import mi_ref
    assert len(R.ADD_SEEDS) >= 4 and len(set(R.ADD_SEEDS)) == len(R.ADD_SEEDS)
    assert hasattr(mi_ref, "mi_autograd")
    for b in range(3):
        Tb, Lb = int(p["T_b"][b]), int(p["L_b"][b])
        assert Lb <= Tb * (p["R"] - 1)
        assert pruned_ref.check_invariants(p["ranges"][b], Tb, Lb, p["R"]) == []


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header_and_the_map():
    declared = I.declared(HEADER)
    assert declared == NAMES
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_ranges.map")).read()
    assert set(re.findall(r"^\s+(\w+);", text, re.M)) == declared
    assert I.exports(_lib()) == declared


def test_the_header_declares_no_sizing_function():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "get_workspace_size" not in text and not any("workspace" in f or "size" in f for f in I.declared(HEADER))
    assert not any(t == "size_t*" for sig in I.declared_signatures(HEADER).values() for t in sig)


def test_other_libraries_export_nothing_of_this_one():
    _lib()
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any(s in NAMES or "ranges_occ" in s or "coverage" in s for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import ranges
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == NAMES and all(sigs.values())
    assert I.binding_faults(ranges.EXPORTS, HEADER) == []
    assert [len(sigs[n]) for n in ("compute_rnnt_prune_ranges_occ", "compute_rnnt_range_coverage")] == [12, 12]


def test_code_objects_hold_exactly_the_kernels():
    I.assert_side_inventory(_lib(), expected_inventory())


def test_the_tile_rule_is_the_kernels():
    """The thresholds the GPU test's shapes straddle (tests/ranges_ref.py tile()) are those of rg_tile."""
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_ranges_kernels.h")).read()
    assert "constexpr int kRgLdsDoubles = 6144;" in text and "constexpr int kRgMaxTile = 32;" in text
    assert "return U | 1;" in text and "while (tf > 1 && tf * rg_stride(U) > kRgLdsDoubles) tf >>= 1;" in text
    assert [R.tile(u) for u in (1, 191, 192, 383, 384, 767, 768, 1535, 1536, 3071, 3072, 4096)] == \
        [32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
    impl = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_ranges_impl.h")).read()
    assert "constexpr int kRgMaxU = 4096;" in impl and "b0 += kGridSamples" in impl


def test_device_code_has_no_scratch():
    """No scratch, no spilled VGPRs (tools/check_kernel_resources.py) in any of the three code objects."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as res
    import check_lattice_lin_isa as guard
    for unit in OBJECTS.values():
        asm = guard.device_asm(None, os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
        assert res.kernels(asm) and res.check(asm) == [], unit


def test_device_code_has_no_atomics():
    for f in ("rnnt_ranges_kernels.h", "rnnt_ranges_impl.h", "rnnt_ranges.hip"):
        assert "atomic" not in open(os.path.join(ROOT, "warp-transducer_amd", "csrc", f)).read().lower(), f


def test_build_lists_name_the_library():
    mk = os.path.join("warp-transducer_amd", "Makefile")
    for path, pattern in (("setup.py", '+ ("ranges",)'), (mk, "SIDE += sample\nSIDE += ranges\n"),
                          (mk, "build/asan/test_ranges_args"), (mk, "SIDE_ARGS := $(filter-out ranges,$(SIDE_ARGS))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS ranges)"), ("MANIFEST.in", "exports_ranges.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_ranges_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_ranges_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_ranges_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_ranges_args" in mk
    assert "build/asan/test_ranges_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_importing_the_package_does_not_load_the_library():
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\nfrom warprnnt_pytorch import ranges\n"
            "assert ranges._LIB._handle is None\n"
            "assert not any('libwarprnnt_ranges' in line for line in open('/proc/self/maps'))\nprint('ok')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]


def test_a_missing_library_is_an_import_error(tmp_path):
    code = ("import sys\nsys.path.insert(0, %r)\nfrom warprnnt_pytorch import ranges\n"
            "try:\n    ranges.lib()\nexcept ImportError as e:\n    print(e)\nelse:\n    sys.exit('loaded something')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WARP_RNNT_PATH=str(tmp_path)), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.strip() == ("libwarprnnt_ranges.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for prune_ranges_from_occupations." % (tmp_path / "libwarprnnt_ranges.so"))


def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import ranges
    px, py = torch.zeros(2, 3, 6), torch.zeros(2, 4, 5)
    rg = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="prune_ranges_from_occupations runs on the GPU only"):
        ranges.prune_ranges_from_occupations(px, py)
    with pytest.raises(ValueError, match="range_coverage runs on the GPU only"):
        ranges.range_coverage(px, py, rg, 3)
    with pytest.raises(ValueError, match="3D tensor"):
        ranges.prune_ranges_from_occupations(px[0], py)
    with pytest.raises(TypeError, match="must be a tensor"):
        ranges.prune_ranges_from_occupations(None, py)
    with pytest.raises(ValueError, match="px_grad must be"):
        ranges.prune_ranges_from_occupations(torch.zeros(2, 3, 7), py)
    with pytest.raises(ValueError, match="px_grad must be"):
        ranges.get_rnnt_prune_ranges(torch.zeros(2, 3, 4), py, None, 3)
    with pytest.raises(TypeError, match="share one dtype"):
        ranges.range_coverage(px.double(), py, rg, 3)
    with pytest.raises(TypeError, match="share one dtype"):
        ranges.prune_ranges_from_occupations(px.long(), py.long())
    with pytest.raises(ValueError, match="contiguous"):
        ranges.prune_ranges_from_occupations(torch.zeros(2, 6, 3).transpose(1, 2), py)
    with pytest.raises(ValueError, match="int64 tensor of shape"):
        ranges.prune_ranges_from_occupations(px, py, torch.zeros(2, 4, dtype=torch.int32))
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="s_range must be an int"):
            ranges._width(bad, 3)
    assert ranges._width(3, 3) == 3 and ranges._width(4, 3) == 4 and ranges._width(9, 3) == 4 and ranges._width(1, 0) == 1
    assert ranges._dims(px, py) == (2, 3, 5, False) and ranges._dims(torch.zeros(2, 3, 5), py) == (2, 3, 5, True)
    assert ranges.__all__ == ["prune_ranges_from_occupations", "get_rnnt_prune_ranges", "range_coverage", "library_path"]
