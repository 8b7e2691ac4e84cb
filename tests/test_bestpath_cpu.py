"""No GPU: the fp64 reference of the best path over px / py (tests/bestpath_ref.py) against brute-force enumeration of every
path and against closed forms; libwarprnnt_bestpath.so's C-ABI, export map and code objects against include/rnnt_bestpath.h
and tests/bestpath_forms.py; the build lists; the argument program under the host sanitizers; and the refusals of
warprnnt_pytorch.bestpath that need no device."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bestpath_forms as F
from tests import bestpath_ref as R
from tests import inventory as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_bestpath.so", "rnnt_bestpath.h"
NEG = float("-inf")


# ----------------------------------------------------------------------------- the reference against enumeration
def _quarters(rng, shape, holes, levels=17):
    """Multiples of 0.25 in [-4, 0] (sums are exact), `levels` of them evenly spaced -- the fewer, the more exact ties --
    with -inf holes."""
    w = -0.25 * (16 // (levels - 1)) * rng.integers(0, levels, size=shape)
    if holes:
        w[rng.random(shape) < 0.12] = NEG
    return w


def _drawn_rectangles():
    """(X, Y, (s0, t0, s1, t1), mod) for S <= 4, T <= 5, both types, sub-rectangles, with and without holes."""
    rng = np.random.default_rng(20)
    out = []
    for k in range(240):
        mod = bool(k % 2)
        S, T = int(rng.integers(2, 4 if mod else 5)), int(rng.integers(4, 6))
        holes = k % 8 >= 6
        levels = (2, 2, 3, 2, 3, 2, 5, 17)[(k // 8) % 8]
        X, Y = _quarters(rng, (S, T if mod else T + 1), holes, levels), _quarters(rng, (S + 1, T), holes, levels)
        s0, t0 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        s1, t1 = int(rng.integers(s0, S + 1)), int(rng.integers(t0, T + 1))
        if k % 3:
            s1, t1 = S, T
        out.append((X, Y, (s0, t0, s1, t1), mod))
    return out


def test_reference_equals_enumeration_and_ties_are_exercised():
    tied = 0
    drawn = _drawn_rectangles()
    for X, Y, bd, mod in drawn:
        s0, t0, s1, t1 = bd
        S, T = Y.shape[0] - 1, Y.shape[1]
        sc, fr, back = R.best_path(X[None], Y[None], np.array([bd]), mod)
        paths = R.brute(X, Y, s0, t0, s1, t1, mod)
        best = max((w for w, _ in paths), default=NEG)
        assert sc[0] == best, (bd, mod, sc, best)                              # exact: quarters
        winners = sorted(f for w, f in paths if w == best and best > NEG)
        tied += len(winners) >= 2
        if best == NEG:
            assert (fr == -1).all()
        else:
            smallest = tuple(min(f[i] for f in winners) for i in range(s1 - s0))
            assert smallest in winners                                         # (the minima form a path of their own)
            assert tuple(fr[0, s0:s1]) == smallest, (bd, mod, fr, winners)
            assert (fr[0, :s0] == -1).all() and (fr[0, s1:] == -1).all()
            inside = fr[0, s0:s1]
            assert (np.diff(inside) >= (1 if mod else 0)).all()
            assert not len(inside) or (t0 <= inside.min() and inside.max() <= (t1 - 1 if mod else t1))
            assert R.rescore(X[None], Y[None], np.array([bd]), mod, fr)[0, 0] == best
        # the strict rule on every reachable node: the bit says "the symbol candidate is strictly better"
        p, bit, bad = R.sweep_one(X, Y, s0, t0, s1, t1, mod)
        assert not bad
        for i in range(s1 - s0 + 1):
            for j in range(t1 - t0 + 1):
                got = bool((int(back[0, s0 + i, (t0 + j) >> 6]) >> ((t0 + j) & 63)) & 1)
                assert got == bool(bit[i, j])
                if p[i, j] > NEG and (i or j):
                    x = p[i - 1, j - 1 if mod else j] + X[s0 + i - 1, t0 + (j - 1 if mod else j)] \
                        if i > 0 and (j > 0 or not mod) else NEG
                    y = p[i, j - 1] + Y[s0 + i, t0 + j - 1] if j > 0 else NEG
                    assert got == (x > y) and p[i, j] == max(x, y)
        # nothing outside the rectangle's nodes
        mask = np.zeros((S + 1, T + 1), bool)
        mask[s0:s1 + 1, t0:t1 + 1] = True
        for s in range(S + 1):
            for t in range(T + 1):
                if not mask[s, t]:
                    assert not (int(back[0, s, t >> 6]) >> (t & 63)) & 1
    assert 3 * tied >= len(drawn), (tied, len(drawn))                          # the tie rule is really exercised


@pytest.mark.parametrize("S", [6, 64])
@pytest.mark.parametrize("mod", [False, True])
def test_the_wrong_tie_rule_differs(S, mod):
    """The reference with `>=` (the symbol edge on ties) -- the negative control of the GPU test -- gives other frames and
    other bits on the tied inputs that test uses, and the same scores."""
    px, py, bd = tie_case(S, mod)
    sc, fr, bk = R.best_path(px, py, bd, mod)
    sc2, fr2, bk2 = R.best_path(px, py, bd, mod, strict=False)
    assert np.isfinite(sc).all() and np.array_equal(sc, sc2)
    assert not np.array_equal(fr, fr2) and not np.array_equal(bk, bk2)


def tie_case(S, mod, N=3):
    """The tied inputs of the device test: (px, py, boundary) with S symbols, room for them in the modified type."""
    T = 70 if mod else 9
    bd = np.array([[0, 0, S, T], [1, 2, S - 1, T - 1], [0, 1, S, T]], np.int64)
    return tie_problem(S, T, mod, N) + (bd,)


def tie_problem(S, T, mod, N=3, seed=5):
    """Multiples of 0.25 in [-0.5, 0], exact in every storage type: nearly every node of the lattice is an exact tie."""
    rng = np.random.default_rng(seed)
    return (-0.25 * rng.integers(0, 3, size=(N, S, T if mod else T + 1)), -0.25 * rng.integers(0, 3, size=(N, S + 1, T)))


@pytest.mark.parametrize("mod", [False, True])
def test_closed_forms(mod):
    S, T = 3, 7
    bd = np.array([[0, 0, 3, 7], [1, 2, 3, 6], [2, 1, 2, 5], [0, 3, 3, 3], [0, 0, 3, 3]], np.int64)
    N = len(bd)
    # uniform weights: every path of a rectangle weighs the same, the tie rule alone decides
    px, py = np.full((N, S, T if mod else T + 1), -0.5), np.full((N, S + 1, T), -0.5)
    sc, fr, _ = R.best_path(px, py, bd, mod)
    for b, (s0, t0, s1, t1) in enumerate(bd):
        if mod and s1 - s0 > t1 - t0:
            assert sc[b] == NEG and (fr[b] == -1).all()
            continue
        n = (t1 - t0) if mod else (s1 - s0) + (t1 - t0)
        assert sc[b] == -0.5 * n
        want = [t0 + (s - s0 if mod else 0) for s in range(s0, s1)]
        assert list(fr[b, s0:s1]) == want and (fr[b, :s0] == -1).all() and (fr[b, s1:] == -1).all()
    # single-path rectangles: s1 == s0 (frames only), t1 == t0 (regular: symbols only), modified s1 - s0 == t1 - t0
    rng = np.random.default_rng(1)
    px, py = rng.standard_normal(px.shape) - 1, rng.standard_normal(py.shape) - 1
    sc, fr, _ = R.best_path(px, py, bd, mod)
    assert sc[2] == np.add.accumulate(py[2, 2, 1:5])[-1] and (fr[2] == -1).all()
    if mod:
        assert sc[3] == NEG
        acc = 0.0
        for i in range(3):
            acc = acc + px[4, i, i]
        assert sc[4] == acc and list(fr[4]) == [0, 1, 2]
    else:
        acc = 0.0
        for i in range(3):
            acc = acc + px[3, i, 3]
        assert sc[3] == acc and list(fr[3]) == [3, 3, 3]
    ex, ey = R.edges(fr, sc, bd, S, T, mod)
    for b in range(N):
        if np.isfinite(sc[b]):
            assert (ex[b] * px[b]).sum() + (ey[b] * py[b]).sum() == pytest.approx(sc[b], rel=1e-14)
        else:
            assert not ex[b].any() and not ey[b].any()
    # S = 0: px has no element
    py0 = rng.standard_normal((2, 1, 9))
    sc, fr, bk = R.best_path(np.zeros((2, 0, 9 if mod else 10)), py0, np.array([[0, 0, 0, 9], [0, 3, 0, 4]]), mod)
    assert sc[0] == np.add.accumulate(py0[0, 0])[-1] and sc[1] == py0[1, 0, 3] and fr.shape == (2, 0) and not bk.any()


def test_reference_edge_cases():
    S, T = 2, 4
    px, py = np.zeros((3, S, T + 1)), np.zeros((3, S + 1, T))
    px[0, 1, :] = NEG                                       # no path
    py[1, 2, 3] = np.nan                                    # poisoned
    bd = np.array([[0, 0, 2, 4], [0, 0, 2, 4], [0, 0, 3, 4]], np.int64)    # the last: outside the tensor
    sc, fr, bk = R.best_path(px, py, bd, False)
    assert sc[0] == NEG and np.isnan(sc[1]) and (fr == -1).all() and not bk[2].any()
    assert sc[2:].view(np.uint64)[0] == 0x7ff8dead00000000
    ex, ey = R.edges(fr, sc, bd, S, T, False)
    assert not ex[0].any() and not ey[0].any() and np.isnan(ex[1]).all() and np.isnan(ey[1]).all()
    assert not ex[2].any() and not ey[2].any()


# ----------------------------------------------------------------------------- the table
def test_the_table_names_every_form_and_threshold():
    us = {c["S"] + 1 for c in F.CASES.values()}
    assert {1, 2, 7, 64, 65, 130, 1100} <= us
    assert all(c["N"] == 2 for c in F.CASES.values() if c["S"] + 1 == 1100)
    for d in ("f32", "f64", "bf16", "f16"):
        mine = [c for c in F.CASES.values() if c["dtype"] == d]
        assert {(F.form(c), c["mod"]) for c in mine} == {(f, m) for f in ((1, False), (1, True), (F.WIDE_ROWS, True))
                                                         for m in (False, True)}
    for d in ("f32", "f64"):
        for mod in (False, True):
            st = {F.steps(c) for c in F.CASES.values() if c["dtype"] == d and c["mod"] == mod and c["S"] == 3}
            assert {F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 3 * F.CHUNK - 1, 3 * F.CHUNK, 3 * F.CHUNK + 1} <= st
    for mod in (False, True):
        assert {62, 63, 64, 65, 127, 128} <= {c["T"] for c in F.CASES.values() if c["mod"] == mod}
    assert any(c["dtype"] == "f32" and c["T"] % 2 for c in F.CASES.values())
    assert any(c["dtype"] in ("bf16", "f16") and c["T"] % 8 for c in F.CASES.values())
    assert F.threads(dict(S=0)) == 64 and F.threads(dict(S=64)) == 128 and F.threads(dict(S=1023)) == 1024
    assert F.threads(dict(S=1099)) == 320 and F.threads(dict(S=4095)) == 1024


def test_the_tables_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_bestpath_kernels.h")).read()
    for name, v in (("kBpChunk", F.CHUNK), ("kBpChunkWide", F.CHUNK_WIDE), ("kBpWideRows", F.WIDE_ROWS),
                    ("kBpWaveMaxU", F.WAVE_MAX_U), ("kBpLdsWords", F.LDS_WORDS)):
        assert "constexpr int %s = %d;" % (name, v) in text, name
    assert "__launch_bounds__(MULTI ? %d : 64)" % F.BLOCK_MAX in text and "__launch_bounds__(%d)" % F.TILE in text
    impl = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_bestpath_impl.h")).read()
    assert "if (U <= kBpWaveMaxU) RNNT_BP_SWEEP(1, false, 64);" in impl
    assert "else if (U <= %d) RNNT_BP_SWEEP(1, true, (U + 63) / 64 * 64);" % F.BLOCK_MAX in impl
    assert "constexpr int kBpMaxU = %d;" % (F.BLOCK_MAX * F.WIDE_ROWS) in impl


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header_and_the_map():
    declared = I.declared(HEADER)
    assert declared == {"compute_rnnt_bestpath", "compute_rnnt_bestpath_edges"}
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_bestpath.map")).read()
    assert set(re.findall(r"^\s+(\w+);", text, re.M)) == declared
    assert I.exports(I.need_lib(LIB)) == declared


def test_the_header_declares_no_sizing_function():
    """The library takes no workspace: the back-pointer bits are an output the caller allocates."""
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "get_workspace_size" not in text and not any("workspace" in f or "size" in f for f in I.declared(HEADER))
    assert not any(t == "size_t*" for sig in I.declared_signatures(HEADER).values() for t in sig)


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any("bestpath" in s for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import bestpath
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(bestpath.EXPORTS, HEADER) == []
    assert len(sigs["compute_rnnt_bestpath"]) == 14 and len(sigs["compute_rnnt_bestpath_edges"]) == 12


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for tag in ("F32", "F64", "BF16", "F16"):
        for mod in ("true", "false"):
            for form in ("1, false", "1, true", "4, true"):
                assert "rnnt::bestpath_sweep_kernel<rnnt::%s, %s, %s>" % (tag, mod, form) in ks
            assert "rnnt::bestpath_edges_kernel<rnnt::%s, %s>" % (tag, mod) in ks
    assert len(ks) == 32


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


def test_build_lists_name_the_library():
    mk = os.path.join("warp-transducer_amd", "Makefile")
    for path, pattern in (("setup.py", '+ ("bestpath",)'), (mk, "SIDE += logprobs\nSIDE += bestpath\n"),
                          (mk, "build/asan/test_bestpath_args"), (mk, "SIDE_ARGS := $(filter-out bestpath,$(SIDE_ARGS))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS bestpath)"), ("MANIFEST.in", "exports_bestpath.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_bestpath_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_bestpath_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_bestpath_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_bestpath_args" in mk
    assert "build/asan/test_bestpath_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_importing_the_package_does_not_load_the_library():
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\nfrom warprnnt_pytorch import bestpath\n"
            "assert bestpath._LIB._handle is None\n"
            "assert not any('libwarprnnt_bestpath' in line for line in open('/proc/self/maps'))\n"
            "assert not hasattr(warprnnt_pytorch, 'best_path')\nprint('ok')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]


def test_a_missing_library_is_an_import_error(tmp_path):
    code = ("import sys\nsys.path.insert(0, %r)\nfrom warprnnt_pytorch import bestpath\n"
            "try:\n    bestpath.lib()\nexcept ImportError as e:\n    print(e)\nelse:\n    sys.exit('loaded something')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WARP_RNNT_PATH=str(tmp_path)), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.strip() == ("libwarprnnt_bestpath.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for best_path." % (tmp_path / "libwarprnnt_bestpath.so"))


def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import bestpath
    px, py = torch.zeros(2, 3, 6), torch.zeros(2, 4, 5)
    with pytest.raises(ValueError, match="best_path runs on the GPU only"):
        bestpath.best_path(px, py)
    with pytest.raises(ValueError, match="3D tensor"):
        bestpath.best_path(px[0], py)
    with pytest.raises(ValueError, match="px must be"):
        bestpath.best_path(torch.zeros(2, 3, 7), py)
    with pytest.raises(ValueError, match="share one dtype"):
        bestpath.best_path(px.double(), py)
    with pytest.raises(ValueError, match="share one dtype"):
        bestpath.best_path(px.long(), py.long())
    with pytest.raises(ValueError, match="contiguous"):
        bestpath.best_path(torch.zeros(2, 6, 3).transpose(1, 2), py)
    with pytest.raises(ValueError, match="int64 tensor of shape"):
        bestpath.best_path(px, py, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64 tensor of shape"):
        bestpath.best_path(px, py, torch.zeros(3, 4, dtype=torch.int64))
    assert bestpath.back_words(62) == 1 and bestpath.back_words(63) == 1 and bestpath.back_words(64) == 2
    assert bestpath.__all__ == ["best_path", "library_path"]
