"""No GPU: the fp64 reference of the fused edge log-probabilities (tests/logprobs_ref.py) against k2's published formulas
(get_rnnt_logprobs_joint, get_rnnt_logprobs_pruned: logsumexp, gathers, permutes, cat, the roll by the window starts and
fix_for_boundary) written out in plain torch fp64 with autograd; libwarprnnt_logprobs.so's C-ABI, export map and code objects
against include/rnnt_logprobs.h and tests/logprobs_forms.py; the build lists; the argument program under the host sanitizers;
and the refusals of warprnnt_pytorch.logprobs that need no device."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import logprobs_forms as F
from tests import logprobs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_logprobs.so", "rnnt_logprobs.h"
INF = float("inf")


# ----------------------------------------------------------------------------- k2's formulas, plain torch
def _fix_for_boundary(px, boundary):
    if boundary is None:
        return px
    B, S, T1 = px.shape
    tb = boundary[:, 3].reshape(B, 1, 1).expand(B, S, T1)
    return px.scatter(2, tb, -INF)


def k2_joint(logits, symbols, blank, boundary, modified):
    B, T, S1, _ = logits.shape
    S = S1 - 1
    norm = torch.logsumexp(logits, dim=3).permute(0, 2, 1)                               # (B, S + 1, T)
    px = torch.gather(logits[:, :, :S], 3, symbols.reshape(B, 1, S, 1).expand(B, T, S, 1)).squeeze(-1).permute(0, 2, 1)
    px = px - norm[:, :S]
    if not modified:
        px = torch.cat((px, torch.full((B, S, 1), -INF, dtype=px.dtype)), dim=2)
    py = logits[:, :, :, blank].permute(0, 2, 1) - norm
    return (px if modified else _fix_for_boundary(px, boundary)), py


def _roll_by_shifts(src, shifts):
    """k2's: out[b, t, (i + shifts[b, t]) % n] = src[b, t, i]."""
    B, T, n = src.shape
    index = (torch.arange(n).view(1, 1, n) - shifts.reshape(B, T, 1)) % n
    return torch.gather(src, 2, index)


def k2_pruned(logits, symbols, ranges, blank, boundary, modified):
    B, T, K, _ = logits.shape
    S = symbols.shape[1]
    norm = torch.logsumexp(logits, dim=3)                                                # (B, T, K)
    with_terminal = torch.cat((symbols, torch.full((B, 1), blank, dtype=symbols.dtype)), dim=1)
    pruned_symbols = torch.gather(with_terminal.unsqueeze(1).expand(B, T, S + 1), 2, ranges)
    px = torch.gather(logits, 3, pruned_symbols.unsqueeze(-1)).squeeze(-1) - norm
    pad = torch.full((B, T, S + 1 - K), -INF, dtype=logits.dtype)
    px = _roll_by_shifts(torch.cat((px, pad), dim=2), ranges[:, :, 0])[:, :, :S].permute(0, 2, 1)
    if not modified:
        px = torch.cat((px, torch.full((B, S, 1), -INF, dtype=px.dtype)), dim=2)
    py = logits[:, :, :, blank] - norm
    py = _roll_by_shifts(torch.cat((py, pad), dim=2), ranges[:, :, 0]).permute(0, 2, 1)
    return (px if modified else _fix_for_boundary(px, boundary)), py


def _problem(seed, K, B=3, T=5, S=3, C=6):
    rng = np.random.default_rng(seed)
    U = S + 1
    case = dict(B=B, T=T, U=U, K=K)
    z = rng.standard_normal((B, T, U if K == 0 else K, C)) * 2
    sym = rng.integers(0, C, size=(B, S))
    sym[0, 0] = 1                                           # (the blank below: a symbol equal to it)
    bd = F.boundary(case, rng)
    rg = F.ranges(case, rng) if K else None
    return rng, z, sym, bd, rg


def _rectangles(px, py, bd):
    """Boolean masks of the elements inside each sample's rectangle: px[b, :S_b, :T_b] -- and, in the regular type, column T_b,
    which k2's fix_for_boundary sets -- and py[b, :S_b + 1, :T_b]."""
    mx, my = np.zeros(px.shape, bool), np.zeros(py.shape, bool)
    regular = px.shape[2] == py.shape[2] + 1
    for b in range(px.shape[0]):
        sb, tb = (px.shape[1], py.shape[2]) if bd is None else (int(bd[b, 2]), int(bd[b, 3]))
        mx[b, :sb, :tb + 1 if regular else tb] = True
        my[b, :sb + 1, :tb] = True
    return mx, my


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("K", [0, 1, 2, 4])
@pytest.mark.parametrize("with_boundary", [True, False])
@pytest.mark.parametrize("seed", range(2))
def test_reference_equals_k2s_formulas(seed, with_boundary, K, modified):
    rng, z, sym, bd, rg = _problem(seed, K)
    if not with_boundary:
        bd = None
    blank = 1
    px, py, lse = R.forward(z, sym, blank, K, rg, bd, modified)
    zt = torch.tensor(z, requires_grad=True)
    tbd = None if bd is None else torch.tensor(bd)
    if K == 0:
        kx, ky = k2_joint(zt, torch.tensor(sym), blank, tbd, modified)
    else:
        k2_ranges = torch.tensor(rg, dtype=torch.int64).unsqueeze(-1) + torch.arange(K)
        kx, ky = k2_pruned(zt, torch.tensor(sym), k2_ranges, blank, tbd, modified)
    mx, my = _rectangles(px, py, bd)
    assert (px[~mx] == -INF).all() and (py[~my] == -INF).all()
    for mine, theirs, m in ((px, kx.detach().numpy(), mx), (py, ky.detach().numpy(), my)):
        a, b = mine[m], theirs[m]
        assert ((a == -INF) == (b == -INF)).all()
        fin = np.isfinite(a)
        assert fin.any() and np.abs(a[fin] - b[fin]).max() <= 1e-12
    # gradients: random weights on the finite elements inside the rectangles, and on lse over the real rows
    wx = np.where(mx & np.isfinite(px), rng.standard_normal(px.shape), 0.0)
    wy = np.where(my & np.isfinite(py), rng.standard_normal(py.shape), 0.0)
    real = R.real_mask(z.shape[0], z.shape[1], sym.shape[1] + 1, K, rg, bd)
    wl = np.where(real, rng.standard_normal(lse.shape), 0.0)
    assert not lse[~real].any()
    zero = torch.zeros((), dtype=torch.float64)
    loss = (torch.where(torch.tensor(wx != 0), kx, zero) * torch.tensor(wx)).sum() \
        + (torch.where(torch.tensor(wy != 0), ky, zero) * torch.tensor(wy)).sum() \
        + (torch.logsumexp(zt, dim=3) * torch.tensor(wl)).sum()
    loss.backward()
    # the incoming gradients hold garbage outside the rectangles: the definition does not read it
    gx = np.where(wx != 0, wx, np.where(mx & np.isfinite(px), 0.0, np.nan))
    gy = np.where(wy != 0, wy, np.where(my & np.isfinite(py), 0.0, np.nan))
    dz, *_ = R.backward(z, lse, sym, blank, gx, gy, np.where(real, wl, np.nan), K, rg, bd, modified)
    assert np.isfinite(dz).all() and not dz[~real].any()
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12


def test_reference_edge_rows():
    """-inf entries beside a finite one behave as torch's log_softmax; an all -inf row, a NaN row and a +inf row poison only
    themselves; a symbol outside [0, C) gives -inf and no gradient."""
    z = np.zeros((1, 4, 2, 3))
    z[0, 0, 0] = [-INF, 0.0, 1.0]
    z[0, 1, 0] = -INF
    z[0, 2, 0, 1] = np.nan
    z[0, 3, 0, 2] = INF
    sym = np.array([[0]])
    px, py, lse = R.forward(z, sym, 1)
    ref = torch.log_softmax(torch.tensor(z[0, 0, 0]), 0).numpy()
    assert px[0, 0, 0] == -INF and abs(py[0, 0, 0] - ref[1]) <= 1e-15
    assert np.isnan(lse[0, 1:, 0]).all() and np.isnan(px[0, 0, 1:4]).all() and np.isnan(py[0, 0, 1:]).all()
    assert np.isfinite(lse[0, :, 1]).all() and np.isfinite(py[0, 1]).all()
    dz, *_ = R.backward(z, lse, sym, 1, np.ones_like(px), np.ones_like(py))
    assert np.isnan(dz[0, 1:, 0]).all() and np.isfinite(dz[0, :, 1]).all() and np.isfinite(dz[0, 0, 0]).all()
    px, _, lse = R.forward(np.zeros((1, 2, 2, 3)), np.array([[3]]), 1)
    assert (px == -INF).all()
    dz, _, gx, _ = R.backward(np.zeros((1, 2, 2, 3)), lse, np.array([[3]]), 1, np.ones_like(px), np.zeros((1, 2, 2)))
    assert not dz.any() and not gx.any()


# ----------------------------------------------------------------------------- the table
def test_the_table_names_every_form_and_threshold():
    for d in ("f32", "f64", "bf16", "f16"):
        mine = [c for c in F.CASES.values() if c["dtype"] == d]
        esz = F.STORES[d][3]
        assert {(F.lanes(c), F.vec(c)) for c in mine} == {(g, v) for g in (4, 16, 64) for v in (True, False)}
        sizes = {c["C"] * esz for c in mine}
        assert {F.NARROW_BYTES, F.NARROW_BYTES + esz, F.WIDE_BYTES, F.WIDE_BYTES + esz} <= sizes
        assert {(c["K"] > 0, c["mod"]) for c in mine} == {(p, m) for p in (False, True) for m in (0, 1)}
        assert any(c["C"] > 4096 for c in mine) and any(c.get("off") for c in mine)
        assert any(c["C"] % 2 and not F.vec(c) for c in mine)


def test_the_tables_thresholds_are_the_kernels():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_logprobs_kernels.h")).read()
    assert "constexpr int kLpNarrowBytes = %d;" % F.NARROW_BYTES in text
    assert "constexpr int kLpWideBytes = %d;" % F.WIDE_BYTES in text
    assert text.count("__launch_bounds__(%d)" % F.TILE) == 3
    impl = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_logprobs_impl.h")).read()
    assert "row_bytes <= static_cast<size_t>(kLpNarrowBytes) ? 4 : row_bytes <= static_cast<size_t>(kLpWideBytes) ? 16 : 64" in impl


def test_the_generators():
    for name, c in F.CASES.items():
        bd = F.boundary(c, np.random.default_rng(1))
        assert bd.shape == (c["B"], 4) and bd.dtype == np.int64 and not bd[:, :2].any(), name
        assert (bd[0, 2], bd[0, 3]) == (c["U"] - 1, c["T"]) and (c["B"] < 2 or bd[1, 3] == 0) and (c["B"] < 3 or bd[2, 2] == 0)
        if c["K"]:
            r = F.ranges(c, np.random.default_rng(1))
            assert r.shape == (c["B"], c["T"]) and r.dtype == np.int32 and r.min() == 0 and r.max() == c["U"] - c["K"], name


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header_and_the_map():
    declared = I.declared(HEADER)
    assert declared == {"compute_rnnt_logprobs_fwd", "compute_rnnt_logprobs_bwd"}
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_logprobs.map")).read()
    assert set(re.findall(r"^\s+(\w+);", text, re.M)) == declared
    assert I.exports(I.need_lib(LIB)) == declared


def test_the_header_declares_no_sizing_function():
    """The library takes no workspace: lse is an output and all the backward needs."""
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "get_workspace_size" not in text and not any("workspace" in f for f in I.declared(HEADER))
    assert not any(t == "size_t*" for sig in I.declared_signatures(HEADER).values() for t in sig)


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any("logprobs" in s for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import logprobs
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(logprobs.EXPORTS, HEADER) == []
    assert len(sigs["compute_rnnt_logprobs_fwd"]) == 15 and len(sigs["compute_rnnt_logprobs_bwd"]) == 17


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for tag in ("F32", "F64", "BF16", "F16"):
        for g in (4, 16, 64):
            assert "rnnt::logprobs_lse_kernel<rnnt::%s, %d>" % (tag, g) in ks
        for v in ("true", "false"):
            assert "rnnt::logprobs_grad_kernel<rnnt::%s, %s>" % (tag, v) in ks
        assert "rnnt::logprobs_edges_kernel<rnnt::%s>" % tag in ks
    assert len(ks) == 24


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
    for path, pattern in (("setup.py", '("logprobs",)'), (mk, "SIDE += joiner\nSIDE += logprobs\n"),
                          (mk, "build/asan/test_logprobs_args"), (mk, "$(filter-out logprobs,$(SIDE_ARGS))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS logprobs)"), ("MANIFEST.in", "exports_logprobs.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_logprobs_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_logprobs_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_logprobs_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_logprobs_args" in mk
    assert "build/asan/test_logprobs_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_importing_the_package_does_not_load_the_library():
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\nfrom warprnnt_pytorch import logprobs\n"
            "assert logprobs._LIB._handle is None\n"
            "assert not any('libwarprnnt_logprobs' in line for line in open('/proc/self/maps'))\n"
            "assert not hasattr(warprnnt_pytorch, 'get_rnnt_logprobs_joint')\nprint('ok')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]


def test_a_missing_library_is_an_import_error(tmp_path):
    code = ("import sys\nsys.path.insert(0, %r)\nfrom warprnnt_pytorch import logprobs\n"
            "try:\n    logprobs.lib()\nexcept ImportError as e:\n    print(e)\nelse:\n    sys.exit('loaded something')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WARP_RNNT_PATH=str(tmp_path)), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.strip() == ("libwarprnnt_logprobs.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for the fused edge log-probabilities."
                                  % (tmp_path / "libwarprnnt_logprobs.so"))


def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import logprobs
    z, zp = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 2, 5)
    sym = torch.zeros(2, 3, dtype=torch.int64)
    rg = torch.zeros(2, 3, dtype=torch.int32)
    for fn in (lambda: logprobs.get_rnnt_logprobs_joint(z, sym, 0),
               lambda: logprobs.get_rnnt_logprobs_joint(z, sym.int(), 0, rnnt_type="modified", return_lse=True, validate=False),
               lambda: logprobs.get_rnnt_logprobs_pruned(zp, sym, rg, 0),
               lambda: logprobs.get_rnnt_logprobs_pruned(zp, sym, rg.long().unsqueeze(-1) + torch.arange(2), 0)):
        with pytest.raises(ValueError, match="GPU only"):
            fn()
    for bad in ("constrained", "Regular", "", None, 1):
        with pytest.raises(ValueError, match="'regular' or 'modified'"):
            logprobs.get_rnnt_logprobs_joint(z, sym, 0, rnnt_type=bad)
        with pytest.raises(ValueError, match="'regular' or 'modified'"):
            logprobs.get_rnnt_logprobs_pruned(zp, sym, rg, 0, rnnt_type=bad)
    with pytest.raises(ValueError, match="4D tensor"):
        logprobs.get_rnnt_logprobs_joint(z[0], sym, 0)
    with pytest.raises(ValueError, match="int32 or int64"):
        logprobs.get_rnnt_logprobs_joint(z, sym.float(), 0)
    with pytest.raises(ValueError, match="needs ranges"):
        logprobs.get_rnnt_logprobs_pruned(zp, sym, None, 0)
    assert logprobs.RNNT_TYPES == {"regular": 0, "modified": 1}
    assert logprobs.__all__ == ["get_rnnt_logprobs_joint", "get_rnnt_logprobs_pruned", "library_path"]
