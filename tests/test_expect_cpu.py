"""No GPU: the fp64 reference of the expected path cost over px / py (tests/expect_ref.py) against brute-force enumeration of
every path, against torch autograd over the enumerated paths and against closed forms; libwarprnnt_expect.so's C-ABI, export
map and code objects against include/rnnt_expect.h and tests/expect_forms.py; the build lists; the argument program under the
host sanitizers; and the refusals of warprnnt_pytorch.expect that need no device."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import expect_forms as F
from tests import expect_ref as R
from tests import inventory as I
from tests import mi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_expect.so", "rnnt_expect.h"
NEG = float("-inf")
NAMES = {"compute_rnnt_expect", "compute_rnnt_expect_fwd", "compute_rnnt_expect_bwd"}


# ----------------------------------------------------------------------------- the reference against enumeration
def _drawn():
    """(X, Y, CX, CY, (s0, t0, s1, t1), mod) for S <= 4, T <= 5: both types, sub-rectangles, -inf edges (with NaN and -inf
    costs on them) and rectangles without a path."""
    rng = np.random.default_rng(21)
    out = []
    for k in range(160):
        mod = bool(k % 2)
        S, T = int(rng.integers(1, 4 if mod else 5)), int(rng.integers(2, 6))
        X, Y = rng.standard_normal((S, T if mod else T + 1)) - 1, rng.standard_normal((S + 1, T)) - 1
        CX, CY = rng.standard_normal(X.shape) * 3, rng.standard_normal(Y.shape) * 3
        if k % 8 >= 5:
            X[rng.random(X.shape) < 0.25] = NEG
            Y[rng.random(Y.shape) < 0.2] = NEG
            CX[X == NEG] = np.nan
            CY[Y == NEG] = NEG
        s0, t0 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        s1, t1 = int(rng.integers(s0, S + 1)), int(rng.integers(t0, T + 1))
        if k % 3:
            s0, t0, s1, t1 = 0, 0, S, T
        out.append((X, Y, CX, CY, (s0, t0, s1, t1), mod))
    return out


def test_recursion_equals_enumeration():
    nopath = holes = 0
    for k, (X, Y, CX, CY, bd, mod) in enumerate(_drawn()):
        ge, gs = (1.0, 0.0) if k % 2 else (1.7, -0.6)
        o = R.expected_cost(X[None], Y[None], CX[None], CY[None], np.array([bd]), mod, [ge], [gs])
        sc, ec, gx, gy, hx, hy = R.enumerate_one(X, Y, CX, CY, bd, mod, ge, gs)
        nopath += sc == NEG
        holes += bool((X == NEG).any())
        assert o["scores"][0] == pytest.approx(sc, rel=1e-12) and o["expect"][0] == pytest.approx(ec, rel=1e-12, abs=1e-13)
        for got, want in ((o["gx"][0], gx), (o["gy"][0], gy), (o["hx"][0], hx), (o["hy"][0], hy)):
            assert np.allclose(got, want, rtol=1e-12, atol=1e-13), (k, bd, mod)
        if sc == NEG:
            assert o["expect"][0] == 0 and not any(o[g].any() for g in ("gx", "gy", "hx", "hy"))
        # nodes: the prefix pairs, (-inf, 0) outside the rectangle's nodes
        s0, t0, s1, t1 = bd
        mask = np.zeros(o["nodes"].shape[1:3], bool)
        mask[s0:s1 + 1, t0:t1 + 1] = True
        assert np.isneginf(o["nodes"][0, ~mask, 0]).all() and not o["nodes"][0, ~mask, 1].any()
        assert o["nodes"][0, s0, t0, 0] == 0 and o["nodes"][0, s0, t0, 1] == 0
        assert o["nodes"][0, s1, t1, 0] == o["scores"][0]
        # the magnitudes bound what they are magnitudes of
        assert abs(o["expect"][0]) <= o["Eabs"][0] * (1 + 1e-12)
        assert (np.abs(o["gx"][0]) <= (abs(ge) * o["magx"][0] + abs(gs) * o["occx"][0]) * (1 + 1e-9) + 1e-300).all()
        assert (np.abs(o["gy"][0]) <= (abs(ge) * o["magy"][0] + abs(gs) * o["occy"][0]) * (1 + 1e-9) + 1e-300).all()
    assert nopath >= 3 and holes >= 20                                         # both are really exercised


def test_gradients_equal_torch_autograd_over_the_paths():
    """d / d(W, C) of sum_paths softmax(W) C, W and C the sums of the edges' weights and costs along a path, by torch fp64
    autograd, equals the four gradients of the reference; d / dW of logsumexp(W) the score's."""
    done = 0
    for X, Y, CX, CY, bd, mod in _drawn()[:60]:
        if (X == NEG).any() or (Y == NEG).any():
            continue
        paths = R.walk(X, Y, CX, CY, *bd, mod)
        if not paths or not paths[0][2]:                                       # (a single node: no edge to differentiate in)
            continue
        tx, ty, tcx, tcy = (torch.tensor(a, requires_grad=True) for a in (X, Y, CX, CY))
        W, Cc = [], []
        for _, _, edges in paths:
            w = c = torch.zeros((), dtype=torch.float64)
            for kind, s, t in edges:
                w = w + (tx if kind == "x" else ty)[s, t]
                c = c + (tcx if kind == "x" else tcy)[s, t]
            W.append(w)
            Cc.append(c)
        W, Cc = torch.stack(W), torch.stack(Cc)
        (1.3 * (torch.softmax(W, 0) * Cc).sum() - 0.4 * torch.logsumexp(W, 0)).backward()
        o = R.expected_cost(X[None], Y[None], CX[None], CY[None], np.array([bd]), mod, [1.3], [-0.4])
        zero = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()              # noqa: E731
        for got, want in ((o["gx"][0], zero(tx)), (o["gy"][0], zero(ty)), (o["hx"][0], zero(tcx)), (o["hy"][0], zero(tcy))):
            assert np.allclose(got, want, rtol=1e-11, atol=1e-13), (bd, mod)
        done += 1
    assert done >= 20


def test_identities():
    rng = np.random.default_rng(4)
    B, S, T = 4, 3, 6
    bd = np.array([[0, 0, 3, 6], [1, 2, 3, 5], [0, 1, 2, 6], [2, 0, 2, 4]], np.int64)
    px, py = rng.standard_normal((B, S, T + 1)) - 1, rng.standard_normal((B, S + 1, T)) - 1
    # cy = 1, cx = 0, regular: every path has t1 - t0 frame edges; a constant cost has no gradient in the weights
    o = R.expected_cost(px, py, np.zeros(px.shape), np.ones(py.shape), bd, False)
    assert np.allclose(o["expect"], bd[:, 3] - bd[:, 1], rtol=1e-12)
    assert np.abs(o["gx"]).max() <= 1e-12 and np.abs(o["gy"]).max() <= 1e-12
    # cx_grad, cy_grad: the occupations of tests/mi_ref.py; the scores its scores
    for mod in (False, True):
        x = px[:, :, :T] if mod else px
        cx, cy = rng.standard_normal(x.shape), rng.standard_normal(py.shape)
        o = R.expected_cost(x, py, cx, cy, bd, mod)
        sc, ox, oy = mi_ref.mi_autograd(x, py, bd)
        assert np.allclose(o["scores"], sc, rtol=1e-12) and np.allclose(o["hx"], ox, rtol=1e-10, atol=1e-14)
        assert np.allclose(o["hy"], oy, rtol=1e-10, atol=1e-14)
        # entropy = score - expect(c = w): uniform weights give log(number of paths); a rectangle with one path gives 0
        u = R.expected_cost(np.full(x.shape, -0.7), np.full(py.shape, -0.7), np.full(x.shape, -0.7), np.full(py.shape, -0.7), bd, mod)
        for b, (s0, t0, s1, t1) in enumerate(bd):
            Sr, Tr = s1 - s0, t1 - t0
            n = math.comb(Tr, Sr) if mod else math.comb(Sr + Tr, Sr)
            assert u["scores"][b] - u["expect"][b] == pytest.approx(math.log(n), abs=1e-12)
        one = R.expected_cost(x, py, x, py, np.array([[2, 0, 2, 4], [0, 3, 3, 6] if mod else [0, 3, 3, 3]] * 2), mod)
        assert np.allclose(one["scores"] - one["expect"], 0, atol=1e-12) and np.isfinite(one["scores"]).all()


def test_reference_edge_cases():
    S, T = 2, 4
    px, py = np.zeros((5, S, T + 1)), np.zeros((5, S + 1, T))
    cx, cy = np.ones(px.shape), np.ones(py.shape)
    px[0, 1, :] = NEG                                       # no path
    py[1, 2, 3] = np.nan                                    # a poisoned weight
    cx[3, 0, 1] = np.inf                                    # a non-finite cost on a finite edge
    cy[4, 0, 0] = np.nan                                    # ... but this one on a -inf edge: never looked at
    py[4, 0, 0] = NEG
    bd = np.array([[0, 0, 2, 4], [0, 0, 2, 4], [0, 0, 3, 4], [0, 0, 2, 4], [0, 0, 2, 4]], np.int64)    # sample 2: outside the tensor
    o = R.expected_cost(px, py, cx, cy, bd, False)
    assert o["scores"][0] == NEG and o["expect"][0] == 0 and not o["gx"][0].any() and not o["hy"][0].any()
    assert np.isnan(o["scores"][1]) and np.isnan(o["expect"][1]) and np.isnan(o["gx"][1]).all() and np.isnan(o["hy"][1]).all()
    assert o["scores"][2:3].view(np.uint64)[0] == 0x7ff8dead00000000 and o["expect"][2] == 0 and not o["gy"][2].any()
    assert np.isfinite(o["scores"][3]) and np.isnan(o["expect"][3])
    assert np.isfinite(o["scores"][4]) and o["expect"][4] == pytest.approx(6.0, rel=1e-12) and o["hy"][4, 0, 0] == 0


# ----------------------------------------------------------------------------- the table
def test_the_table_names_every_form_and_threshold():
    us = {c["S"] + 1 for c in F.CASES.values()}
    assert {1, 2, 7, 64, 65, 130, 1024} <= us
    assert all(c["N"] == 2 for c in F.CASES.values() if c["S"] + 1 == 1024)
    for d in ("f32", "f64", "bf16", "f16"):
        mine = [c for c in F.CASES.values() if c["dtype"] == d]
        assert {(F.multi(c), c["mod"]) for c in mine} == {(f, m) for f in (False, True) for m in (False, True)}
    for d in ("f32", "f64"):
        for mod in (False, True):
            st = {F.steps(c) for c in F.CASES.values() if c["dtype"] == d and c["mod"] == mod and c["S"] in (1, 3)}
            assert {F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 3 * F.CHUNK - 1, 3 * F.CHUNK, 3 * F.CHUNK + 1} <= st
    for mod in (False, True):
        assert {1, 2, 62, 63, 64, 65, 127, 128} <= {c["T"] for c in F.CASES.values() if c["mod"] == mod}
    assert any(c["dtype"] == "f32" and c["T"] % 2 for c in F.CASES.values())
    assert any(c["dtype"] in ("bf16", "f16") and c["T"] % 8 for c in F.CASES.values())
    assert F.threads(dict(S=0)) == 64 and F.threads(dict(S=63)) == 64 and F.threads(dict(S=64)) == 128
    assert F.threads(dict(S=1023)) == 1024


def test_the_tables_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_expect_kernels.h")).read()
    for name, v in (("kExChunk", F.CHUNK), ("kExChunkBwd", F.CHUNK_BWD), ("kExWaveMaxU", F.WAVE_MAX_U)):
        assert "constexpr int %s = %d;" % (name, v) in text, name
    assert text.count("__launch_bounds__(MULTI ? %d : 64)" % F.BLOCK_MAX) == 2
    impl = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_expect_impl.h")).read()
    assert "if (U <= kExWaveMaxU) RNNT_EX_FWD(false, 64);" in impl and "else RNNT_EX_FWD(true, (U + 63) / 64 * 64);" in impl
    assert "if (U <= kExWaveMaxU) RNNT_EX_BWD(false, 64);" in impl and "else RNNT_EX_BWD(true, (U + 63) / 64 * 64);" in impl
    assert "constexpr int kExMaxU = %d;" % F.BLOCK_MAX in impl


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header_and_the_map():
    declared = I.declared(HEADER)
    assert declared == NAMES
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_expect.map")).read()
    assert set(re.findall(r"^\s+(\w+);", text, re.M)) == declared
    assert I.exports(I.need_lib(LIB)) == declared
    assert not any(bad in n for n in declared for bad in ("_kd", "bestpath", "logprobs", "joiner"))


def test_the_header_declares_no_sizing_function():
    """The library takes no workspace: `nodes` is an output the caller allocates."""
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "get_workspace_size" not in text and not any("workspace" in f or "size" in f for f in I.declared(HEADER))
    assert not any(t == "size_t*" for sig in I.declared_signatures(HEADER).values() for t in sig)


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any("expect" in s for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import expect
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(expect.EXPORTS, HEADER) == []
    assert [len(sigs[n]) for n in ("compute_rnnt_expect", "compute_rnnt_expect_fwd", "compute_rnnt_expect_bwd")] == [18, 14, 20]


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = set(F.predicted_rows()) | set(F.UNREACHABLE)
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for tag in ("F32", "F64", "BF16", "F16"):
        for mod in ("true", "false"):
            for multi in ("true", "false"):
                assert "rnnt::expect_fwd_kernel<rnnt::%s, %s, %s>" % (tag, mod, multi) in ks
                for wcg in ("true", "false"):
                    assert "rnnt::expect_bwd_kernel<rnnt::%s, %s, %s, %s>" % (tag, mod, multi, wcg) in ks
        assert "rnnt::expect_restore_kernel<rnnt::%s>" % tag in ks
    assert len(ks) == 52


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
    for path, pattern in (("setup.py", '+ ("expect",)'), (mk, "SIDE += bestpath\nSIDE += expect\n"),
                          (mk, "build/asan/test_expect_args"), (mk, "SIDE_ARGS := $(filter-out expect,$(SIDE_ARGS))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS expect)"), ("MANIFEST.in", "exports_expect.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_expect_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_expect_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_expect_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_expect_args" in mk
    assert "build/asan/test_expect_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_importing_the_package_does_not_load_the_library():
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\nfrom warprnnt_pytorch import expect\n"
            "assert expect._LIB._handle is None\n"
            "assert not any('libwarprnnt_expect' in line for line in open('/proc/self/maps'))\n"
            "assert not hasattr(warprnnt_pytorch, 'expected_cost')\nprint('ok')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]


def test_a_missing_library_is_an_import_error(tmp_path):
    code = ("import sys\nsys.path.insert(0, %r)\nfrom warprnnt_pytorch import expect\n"
            "try:\n    expect.lib()\nexcept ImportError as e:\n    print(e)\nelse:\n    sys.exit('loaded something')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WARP_RNNT_PATH=str(tmp_path)), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.strip() == ("libwarprnnt_expect.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for expected_cost." % (tmp_path / "libwarprnnt_expect.so"))


def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import expect
    px, py = torch.zeros(2, 3, 6), torch.zeros(2, 4, 5)
    cx, cy = torch.zeros_like(px), torch.zeros_like(py)
    with pytest.raises(ValueError, match="expected_cost runs on the GPU only"):
        expect.expected_cost(px, py, cx, cy)
    with pytest.raises(ValueError, match="expected_cost runs on the GPU only"):
        expect.alignment_entropy(px, py)
    with pytest.raises(ValueError, match="3D tensor"):
        expect.expected_cost(px[0], py, cx, cy)
    with pytest.raises(ValueError, match="px must be"):
        expect.expected_cost(torch.zeros(2, 3, 7), py, cx, cy)
    with pytest.raises(ValueError, match="share one dtype"):
        expect.expected_cost(px.double(), py, cx, cy)
    with pytest.raises(ValueError, match="contiguous"):
        expect.expected_cost(torch.zeros(2, 6, 3).transpose(1, 2), py, cx, cy)
    with pytest.raises(ValueError, match="int64 tensor of shape"):
        expect.expected_cost(px, py, cx, cy, torch.zeros(2, 4, dtype=torch.int32))
    # the cost tensors against their weight tensors: shape, dtype, layout, device (checked before anything runs)
    meta = lambda t: torch.empty_like(t, device="meta")                                      # noqa: E731
    for bad_cx, bad_cy, msg in ((torch.zeros(2, 3, 5), cy, "shape and dtype of px"), (cx, torch.zeros(2, 4, 6), "shape and dtype of py"),
                                (cx.double(), cy, "shape and dtype of px"), (cx, cy.half(), "shape and dtype of py"),
                                (None, cy, "shape and dtype of px"),
                                (torch.zeros(2, 6, 3).transpose(1, 2), cy, "cx and cy must be contiguous"),
                                (meta(cx), cy, "device of px"), (cx, meta(cy), "device of px")):
        with pytest.raises(ValueError, match=msg):
            expect._certify_costs(px, py, bad_cx, bad_cy)
    expect._certify_costs(px, py, cx, cy)
    expect._certify_costs(px, py, px, py)                                                    # costs may alias the weights
    assert expect.__all__ == ["expected_cost", "alignment_entropy", "library_path"]
