"""No GPU: the fp64 reference of the alignment sampler over px / py (tests/sample_ref.py) against brute-force enumeration of
every path and against torch autograd over the paths' edges; the seeds of tests/sample_forms.py against the decision margin;
libwarprnnt_sample.so's C-ABI, export map and code objects against include/rnnt_sample.h and tests/sample_forms.py; the build
lists; the argument program under the host sanitizers; and the refusals of warprnnt_pytorch.sample that need no device."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bestpath_ref
from tests import expect_ref
from tests import inventory as I
from tests import mi_ref
from tests import sample_forms as F
from tests import sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_sample.so", "rnnt_sample.h"
NEG = float("-inf")
NAMES = {"compute_rnnt_sample", "compute_rnnt_sample_walk", "compute_rnnt_path_weights", "compute_rnnt_path_edges"}


# ----------------------------------------------------------------------------- the reference against enumeration
def _drawn():
    """(X, Y, (s0, t0, s1, t1), mod) for S <= 4, T <= 5: both types, sub-rectangles, -inf edges and rectangles without a
    path."""
    rng = np.random.default_rng(22)
    out = []
    for k in range(160):
        mod = bool(k % 2)
        S, T = int(rng.integers(1, 4 if mod else 5)), int(rng.integers(2, 6))
        X, Y = rng.standard_normal((S, T if mod else T + 1)) - 1, rng.standard_normal((S + 1, T)) - 1
        if k % 8 >= 5:
            X[rng.random(X.shape) < 0.25] = NEG
            Y[rng.random(Y.shape) < 0.2] = NEG
        s0, t0 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        s1, t1 = int(rng.integers(s0, S + 1)), int(rng.integers(t0, T + 1))
        if k % 3:
            s0, t0, s1, t1 = 0, 0, S, T
        out.append((X, Y, (s0, t0, s1, t1), mod))
    return out


def _frames_of(edges, S):
    row = np.full(S, -1, np.int32)
    for kind, s, t in edges:
        if kind == "x":
            row[s] = t
    return row


def test_the_walk_is_an_exact_sampler():
    """For every enumerated path the product of the shares along it is exp(W - score) to 1e-12: the identity that makes the
    sampler exact.  alpha is expect's nodes[..., 0], the score mi's; every drawn walk is one of the enumerated paths and its
    weight the path's, bit for bit."""
    nopath = holes = paths_seen = 0
    rng = np.random.default_rng(5)
    for X, Y, bd, mod in _drawn():
        s0, t0, s1, t1 = bd
        S, T = X.shape[0], Y.shape[1]
        U = rng.random((1, 9, S + T), dtype=np.float32)
        o = R.sample(X[None], Y[None], U, np.array([bd]), mod)
        paths = expect_ref.walk(X, Y, np.zeros(X.shape), np.zeros(Y.shape), s0, t0, s1, t1, mod)
        e = expect_ref.expected_cost(X[None], Y[None], np.zeros((1,) + X.shape), np.zeros((1,) + Y.shape), np.array([bd]), mod)
        assert np.array_equal(np.isneginf(o["alpha"]), np.isneginf(e["nodes"][..., 0]))
        fin = np.isfinite(o["alpha"])
        assert np.allclose(o["alpha"][fin], e["nodes"][..., 0][fin], rtol=1e-12, atol=1e-12)
        sc = mi_ref.mi_autograd(X[None], Y[None], np.array([bd]))[0][0]
        assert (o["scores"][0] == NEG and sc == NEG) or o["scores"][0] == pytest.approx(sc, rel=1e-12, abs=1e-12)
        holes += bool((X == NEG).any())
        if not paths:
            nopath += 1
            assert o["scores"][0] == NEG and (o["frames"] == -1).all() and np.isneginf(o["weights"]).all()
            continue
        a = o["alpha"][0]
        total = 0.0
        for w, _, edges in paths:
            prod = 1.0
            for kind, s, t in edges:                     # the edge INTO node v
                vs, vt = (s + 1, t + 1 if mod else t) if kind == "x" else (s, t + 1)
                if vs == s0:
                    continue                             # no decision: the frame edge
                tp = vt - 1 if mod else vt
                r = np.exp(a[vs - 1, tp] + X[vs - 1, tp] - a[vs, vt]) if tp >= t0 else 0.0
                prod *= r if kind == "x" else 1.0 - r
            assert prod == pytest.approx(np.exp(w - o["scores"][0]), rel=1e-12, abs=1e-15), (bd, mod)
            total += prod
            paths_seen += 1
        assert total == pytest.approx(1.0, rel=1e-12)
        legal = {tuple(_frames_of(edges, S)): w for w, _, edges in paths}
        W, n, _ = R.path_weights(X[None], Y[None], o["frames"], np.array([bd]), mod)
        assert np.array_equal(W, o["weights"])          # the same additions in the same order
        for k in range(9):
            assert tuple(o["frames"][0, k]) in legal
            assert o["weights"][0, k] == pytest.approx(legal[tuple(o["frames"][0, k])], rel=1e-12, abs=1e-12)
            assert R.is_path(o["frames"][0, k], *bd, mod)
    assert nopath >= 3 and holes >= 20 and paths_seen > 500


def test_sampled_frequencies_follow_the_posterior():
    """Not needed for exactness (the identity above is); a sanity check of the walk's use of its uniforms: 20000 walks of one
    small lattice against the enumerated posterior, at 5 standard deviations."""
    rng = np.random.default_rng(8)
    for mod in (False, True):
        S, T = 2, 4
        X, Y = rng.standard_normal((S, T if mod else T + 1)) - 1, rng.standard_normal((S + 1, T)) - 1
        paths = expect_ref.walk(X, Y, np.zeros(X.shape), np.zeros(Y.shape), 0, 0, S, T, mod)
        w = np.array([p[0] for p in paths])
        post = np.exp(w - np.logaddexp.reduce(w))
        index = {tuple(_frames_of(p[2], S)): i for i, p in enumerate(paths)}
        K = 20000
        o = R.sample(X[None], Y[None], rng.random((1, K, S + T), dtype=np.float32), None, mod)
        counts = np.bincount([index[tuple(f)] for f in o["frames"][0]], minlength=len(paths))
        assert (np.abs(counts - K * post) <= 5 * np.sqrt(K * post * (1 - post)) + 1).all()


def test_path_edges_are_the_indicator_and_the_gradient():
    done = 0
    rng = np.random.default_rng(9)
    for X, Y, bd, mod in _drawn()[:80]:
        s0, t0, s1, t1 = bd
        S, T = X.shape[0], Y.shape[1]
        paths = bestpath_ref.brute(X, Y, s0, t0, s1, t1, mod)
        if not paths:
            continue
        rows = []
        for _, fr in paths[:5]:
            row = np.full(S, -1, np.int32)
            row[s0:s1] = fr
            rows.append(row)
        frames = np.array(rows)[None]
        K = frames.shape[1]
        # one path, coeff = 1: bestpath's indicator
        ex, ey = bestpath_ref.edges(frames[:, 0], np.zeros(1), np.array([bd]), S, T, mod)
        gx, gy = R.path_edges(frames[:, :1], None, np.array([bd]), S, T, mod)
        assert np.array_equal(gx, ex) and np.array_equal(gy, ey)
        # d / d(px, py) of sum_k c_k W_k by torch fp64 autograd over the paths' edges
        c = rng.standard_normal((1, K))
        Xf, Yf = np.where(np.isfinite(X), X, -30.0), np.where(np.isfinite(Y), Y, -30.0)
        tx, ty = torch.tensor(Xf, requires_grad=True), torch.tensor(Yf, requires_grad=True)
        loss = torch.zeros((), dtype=torch.float64)
        for k in range(K):
            row, t = frames[0, k], t0
            for s in range(s0, s1 + 1):
                hi = t1 if s == s1 else int(row[s])
                loss = loss + c[0, k] * ty[s, t:hi].sum()
                if s < s1:
                    loss = loss + c[0, k] * tx[s, hi]
                    t = hi + 1 if mod else hi
        if loss.requires_grad:
            loss.backward()
        zero = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()              # noqa: E731
        gx, gy = R.path_edges(frames, c, np.array([bd]), S, T, mod)
        assert np.allclose(gx[0], zero(tx), rtol=1e-13, atol=1e-15) and np.allclose(gy[0], zero(ty), rtol=1e-13, atol=1e-15)
        W, n, sa = R.path_weights(Xf[None], Yf[None], frames, np.array([bd]), mod)
        assert np.allclose(W[0], [p[0] for p in bestpath_ref.brute(Xf, Yf, s0, t0, s1, t1, mod)[:5]], rtol=1e-13, atol=1e-13)
        done += 1
    assert done >= 40


def test_rows_that_are_no_path():
    S, T = 3, 5
    full = (0, 0, S, T)
    for mod, good, bads in ((False, [0, 2, 2], ([0, -1, 2], [2, 1, 3], [0, 2, 6], [-1, -1, -1])),
                            (True, [0, 2, 4], ([0, 2, 2], [0, 2, 5], [1, 0, 3], [0, -1, 3]))):
        assert R.is_path(np.array(good), *full, mod)
        for bad in bads:
            assert not R.is_path(np.array(bad), *full, mod), (mod, bad)
    assert R.is_path(np.array([-1, -1, -1]), 1, 2, 1, 4, False) and R.is_path(np.array([-1, -1, -1]), 2, 0, 2, 0, True)
    assert R.is_path(np.array([-7, 3, 9]), 1, 2, 2, 4, False)              # outside [s0, s1): not looked at
    X, Y = np.zeros((1, S, T + 1)), np.ones((1, S + 1, T))
    fr = np.array([[[0, 2, 2], [2, 1, 3]]], np.int32)
    W, n, sa = R.path_weights(X, Y, fr, None, False)
    assert W[0, 0] == 5 and n[0, 0] == 8 and np.isnan(W[0, 1])
    gx, gy = R.path_edges(fr, np.array([[2.0, np.nan]]), None, S, T, False)
    assert gx.sum() == 6 and gy.sum() == 10 and not np.isnan(gx).any()
    W, _, _ = R.path_weights(X, Y, fr, np.array([[0, 0, S + 1, T]]), False)
    assert np.isnan(W).all()
    o = R.sample(X, Y, np.zeros((1, 2, S + T), np.float32), np.array([[0, 0, S + 1, T]]), False)
    assert o["scores"].view(np.uint64)[0] == 0x7ff8dead00000000 and (o["frames"] == -1).all() and np.isnan(o["weights"]).all()
    assert np.isneginf(o["alpha"]).all()
    # S = 0: no symbol, frames has no element
    Y0 = np.arange(4.0).reshape(1, 1, 4)
    W, n, _ = R.path_weights(np.zeros((1, 0, 5)), Y0, np.zeros((1, 2, 0), np.int32), np.array([[0, 1, 0, 3]]), False)
    assert (W == 3).all() and (n == 2).all()
    gx, gy = R.path_edges(np.zeros((1, 2, 0), np.int32), None, np.array([[0, 1, 0, 3]]), 0, 4, False)
    assert gx.size == 0 and np.array_equal(gy[0, 0], [0, 2, 2, 0])


# ----------------------------------------------------------------------------- the table
def test_the_table_names_every_form_and_threshold():
    us = {c["S"] + 1 for c in F.CASES.values()}
    assert {1, 2, 7, 64, 65, 130, 1024} <= us
    assert all(c["N"] == 2 for c in F.CASES.values() if c["S"] + 1 == 1024)
    assert all(c["N"] == 7 for c in F.CASES.values() if c["S"] + 1 != 1024)
    for d in ("f32", "f64", "bf16", "f16"):
        mine = [c for c in F.CASES.values() if c["dtype"] == d]
        assert {(F.multi(c), c["mod"]) for c in mine} == {(f, m) for f in (False, True) for m in (False, True)}
        assert {c["S"] + 1 for c in mine} >= {7, 65, 1024}
    for d in ("f32", "f64"):
        for mod in (False, True):
            mine = [c for c in F.CASES.values() if c["dtype"] == d and c["mod"] == mod]
            ch = F.chunk(mine[0])
            st = {F.steps(c) for c in mine if c["S"] in (1, 3)}
            assert {ch - 1, ch, ch + 1, 3 * ch - 1, 3 * ch, 3 * ch + 1} <= st
            assert {1, 2, 64, 130} <= {c["S"] + 1 for c in mine}
    for mod in (False, True):
        assert {1, 2, 63, 64, 65} <= {c["T"] for c in F.CASES.values() if c["mod"] == mod}
        assert set(F.KS) <= {c["K"] for c in F.CASES.values() if c["mod"] == mod}
    assert set(F.KS) == {1, 3, 64, 65, 130}
    assert {F.walk_block(k) for k in F.KS} == {64, 128, 192} and F.walk_block(1024) == 256 and F.walk_block(256) == 256
    assert F.threads(dict(S=0)) == 64 and F.threads(dict(S=63)) == 64 and F.threads(dict(S=64)) == 128
    assert F.threads(dict(S=1023)) == 1024


def test_the_tables_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_sample_kernels.h")).read()
    for name, v in (("kSaChunk", F.CHUNK), ("kSaWaveMaxU", F.WAVE_MAX_U), ("kSaMaxK", F.MAX_K), ("kSaWalkBlock", F.WALK_BLOCK)):
        assert "constexpr int %s = %d;" % (name, v) in text, name
    assert text.count("__launch_bounds__(MULTI ? %d : 64)" % F.BLOCK_MAX) == 1
    assert "sizeof(typename Tag::store) == 8 ? kSaChunk / 2 : kSaChunk" in text
    impl = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_sample_impl.h")).read()
    assert "if (U <= kSaWaveMaxU) RNNT_SA_FWD(false, 64);" in impl and "else RNNT_SA_FWD(true, (U + 63) / 64 * 64);" in impl
    assert "const int block = c.K >= kSaWalkBlock ? kSaWalkBlock : (c.K + 63) / 64 * 64;" in impl
    assert "constexpr int kSaMaxU = %d;" % F.BLOCK_MAX in impl


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_every_decision_is_clear(name):
    """Every decision of the reference walks of the case has |u - r| > m, m = sample_ref.margin of the case's sweep: the
    device, whose r differs from the reference's by at most m, then makes the same decision.  A case that fails gets another
    seed in sample_forms.SEEDS, here on the CPU; none is dropped."""
    case = F.CASES[name]
    px, py, bd, _, _, U = F.problem(case)
    o = R.sample(px.double().numpy(), py.double().numpy(), U, bd, case["mod"])
    decided = 0
    for b in range(case["N"]):
        m = R.margin(F.steps(case), o["amax"][b])
        assert m < 1e-6
        assert o["gap"][b] > m, (name, b, o["gap"][b], m)
        decided += np.isfinite(o["gap"][b])
    assert decided or case["S"] == 0
    # 1e-9 (1 + |a|), the GPU test's bound on alpha, covers the sweep's error as derived in sample_ref.margin
    assert 8 * F.steps(case) * R.EPS < 1e-9


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header_and_the_map():
    declared = I.declared(HEADER)
    assert declared == NAMES
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_sample.map")).read()
    assert set(re.findall(r"^\s+(\w+);", text, re.M)) == declared
    assert I.exports(I.need_lib(LIB)) == declared


def test_the_header_declares_no_sizing_function():
    """The library takes no workspace: alpha is an output the caller allocates."""
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "get_workspace_size" not in text and not any("workspace" in f or "size" in f for f in I.declared(HEADER))
    assert not any(t == "size_t*" for sig in I.declared_signatures(HEADER).values() for t in sig)


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any("sample" in s or s in NAMES for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import sample
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(sample.EXPORTS, HEADER) == []
    assert [len(sigs[n]) for n in ("compute_rnnt_sample", "compute_rnnt_sample_walk", "compute_rnnt_path_weights",
                                   "compute_rnnt_path_edges")] == [15, 15, 12, 12]


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
                assert "rnnt::sample_fwd_kernel<rnnt::%s, %s, %s>" % (tag, mod, multi) in ks
            for kernel in ("sample_walk_kernel", "path_weights_kernel", "path_edges_kernel"):
                assert "rnnt::%s<rnnt::%s, %s>" % (kernel, tag, mod) in ks
    assert len(ks) == 40


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
    for path, pattern in (("setup.py", '+ ("sample",)'), (mk, "SIDE += expect\nSIDE += sample\n"),
                          (mk, "build/asan/test_sample_args"), (mk, "SIDE_ARGS := $(filter-out sample,$(SIDE_ARGS))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS sample)"), ("MANIFEST.in", "exports_sample.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_sample_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_sample_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_sample_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_sample_args" in mk
    assert "build/asan/test_sample_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_importing_the_package_does_not_load_the_library():
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\nfrom warprnnt_pytorch import sample\n"
            "assert sample._LIB._handle is None\n"
            "assert not any('libwarprnnt_sample' in line for line in open('/proc/self/maps'))\n"
            "assert not hasattr(warprnnt_pytorch, 'sample_paths')\nprint('ok')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]


def test_a_missing_library_is_an_import_error(tmp_path):
    code = ("import sys\nsys.path.insert(0, %r)\nfrom warprnnt_pytorch import sample\n"
            "try:\n    sample.lib()\nexcept ImportError as e:\n    print(e)\nelse:\n    sys.exit('loaded something')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WARP_RNNT_PATH=str(tmp_path)), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.strip() == ("libwarprnnt_sample.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for sample_paths." % (tmp_path / "libwarprnnt_sample.so"))


def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import sample
    px, py = torch.zeros(2, 3, 6), torch.zeros(2, 4, 5)
    fr = torch.zeros(2, 4, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="sample_paths runs on the GPU only"):
        sample.sample_paths(px, py, 4)
    with pytest.raises(ValueError, match="path_scores runs on the GPU only"):
        sample.path_scores(px, py, fr)
    with pytest.raises(ValueError, match="3D tensor"):
        sample.sample_paths(px[0], py, 4)
    with pytest.raises(ValueError, match="px must be"):
        sample.sample_paths(torch.zeros(2, 3, 7), py, 4)
    with pytest.raises(ValueError, match="share one dtype"):
        sample.path_scores(px.double(), py, fr)
    with pytest.raises(ValueError, match="contiguous"):
        sample.sample_paths(torch.zeros(2, 6, 3).transpose(1, 2), py, 4)
    with pytest.raises(ValueError, match="int64 tensor of shape"):
        sample.sample_paths(px, py, 4, torch.zeros(2, 4, dtype=torch.int32))
    for bad in (0, -1, 1025, 2.0, True, None):
        with pytest.raises(ValueError, match="num_samples must be an int"):
            sample._certify_samples(bad)
    sample._certify_samples(1)
    sample._certify_samples(1024)
    meta = lambda t: torch.empty_like(t, device="meta")                                      # noqa: E731
    u = torch.zeros(2, 4, 8)
    for bad, msg in ((torch.zeros(2, 4, 9), "shape"), (torch.zeros(2, 3, 8), "shape"), (u.double(), "float32"), (None, "float32"),
                     (torch.zeros(2, 8, 4).transpose(1, 2), "contiguous"), (meta(u), "device of px")):
        with pytest.raises(ValueError, match=msg):
            sample._certify_uniforms(bad, py, 4)
    sample._certify_uniforms(u, py, 4)
    for bad, msg in ((fr.long(), "int32"), (torch.zeros(2, 4, 4, dtype=torch.int32), "shape"),
                     (torch.zeros(3, 4, 3, dtype=torch.int32), "shape"), (torch.zeros(2, 0, 3, dtype=torch.int32), "between 1 and"),
                     (torch.zeros(2, 1025, 3, dtype=torch.int32), "between 1 and"),
                     (torch.zeros(2, 3, 4, dtype=torch.int32).transpose(1, 2), "contiguous"), (meta(fr), "device of px"),
                     (None, "int32")):
        with pytest.raises(ValueError, match=msg):
            sample._certify_frames(bad, py)
    assert sample._certify_frames(fr, py)[1] == 4
    f2, k = sample._certify_frames(fr[:, 0].contiguous(), py)
    assert k == 1 and tuple(f2.shape) == (2, 1, 3)
    assert sample.__all__ == ["sample_paths", "path_scores", "library_path"]
