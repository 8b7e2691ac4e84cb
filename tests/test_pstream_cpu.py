"""No GPU: the fp64 reference of the pruned loss with lattice type and delay penalty (tests/pstream_ref.py) against
brute-force path enumeration, against the references of the three libraries it must agree with (tests/pruned_ref.py at type 0
and penalty 0; tests/delay_ref.py and tests/mono_ref.py on the materialised tensor) and against the px / py recursion of
tests/mi_ref.py under the k2 mapping; the windows generator against brute-force reachability for every case of
tests/pstream_forms.py; libwarprnnt_pstream.so's C-ABI and code objects against include/rnnt_pstream.h and the table; the build
lists; the argument program under the host sanitizers; and the refusals of warprnnt_pytorch.pstream that need no device."""
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import pstream_forms as F
from tests import pstream_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_pstream.so", "rnnt_pstream.h"


def _tiny(seed, typ, N=5, max_t=6, max_l=3):
    """Lattices up to T = 6, L = 3 with windows around a valid path.  Sample 0 full, sample 1 with T_b = 1, sample 2 with
    L_b = 0, sample 3 with T_b = 1 and L_b >= 1 where the windows allow; labels over all of [0, A), the blank included;
    penalties of both signs."""
    rng = np.random.default_rng(9000 + 97 * typ + seed)
    U = int(rng.integers(1, max_l + 2))
    S = int(rng.integers(1, U + 1))
    lo = max(2, U - 1 if typ else -(-(U - 1) // max(S - 1, 1)))          # frames enough for the full sample's labels
    T = int(rng.integers(min(lo, max_t), max_t + 1))
    A = int(rng.integers(3, 8))
    case = dict(N=N, T=T, U=U, S=S, type=typ)
    tl, ll = F.lengths(case, rng)
    s = F.ranges(case, tl, ll, rng)
    blank = (0, A - 1, A // 2)[seed % 3]
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    x = rng.standard_normal((N, T, S, A)) * 1.5
    penalty = (0.3, -0.7, 0.05, 1.5)[seed % 4]
    return x, labels, s, tl, ll, blank, penalty, S, rng


@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_brute_force(seed, typ):
    x, labels, s, tl, ll, blank, penalty, S, rng = _tiny(seed, typ)
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.pstream_autograd(x, labels, s, tl, ll, blank, typ, penalty, w)
    c2, g2 = R.pstream_brute(x, labels, s, tl, ll, blank, typ, penalty, w)
    assert np.isfinite(c1).all()
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    read = R.read_mask(x.shape, s, tl, ll, typ)
    assert not g1[~read].any() and g1[read].any()
    assert tl[1] == 1 and ll[2] == 0 and tl[F.FRAME_ZERO] == 1


def test_the_tiny_problems_cover_the_listed_cases():
    seen = {"blank_label": 0, "negative": 0, "frame_zero_label": 0}
    for typ in (0, 1):
        for seed in range(40):
            x, labels, s, tl, ll, blank, penalty, S, _ = _tiny(seed, typ)
            seen["blank_label"] += any(blank in labels[b, :ll[b]] for b in range(len(tl)))
            seen["negative"] += penalty < 0
            seen["frame_zero_label"] += ll[F.FRAME_ZERO] >= 1
    assert all(v >= 5 for v in seen.values()), seen


@pytest.mark.parametrize("typ", [0, 1])
def test_windows_without_a_path_cost_infinity(typ):
    """Separating windows, and in the modified type T_b < L_b: both references say +inf and has_path says no."""
    rng = np.random.default_rng(5)
    T, L, S, A = 5, 4, 2, 6
    x = rng.standard_normal((1, T, S, A))
    labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
    s = np.array([[0, 0, 3, 3, 3]], np.int32)                       # states {0, 1} then {3, 4}: no edge out of {0, 1} lands there
    assert not R.has_path(s[0], T, L, S, typ)
    for fn in (R.pstream_autograd, R.pstream_brute):
        c, g = fn(x, labels, s, [T], [L], 0, typ, 0.2)
        assert np.isposinf(c).all() and not g.any()
    if typ == 1:
        s2 = np.zeros((1, 2), np.int32)
        assert not R.has_path(s2[0], 2, 3, 4, 1)
        c, _ = R.pstream_autograd(rng.standard_normal((1, 2, 4, A)), labels, s2, [2], [3], 0, 1, 0.0)
        assert np.isposinf(c).all()


# ----------------------------------------------------------------------------- the identities of the header
@pytest.mark.parametrize("seed", range(8))
def test_type_0_penalty_0_is_the_pruned_reference(seed):
    from tests import pruned_ref
    x, labels, s, tl, ll, blank, _, S, rng = _tiny(seed, 0)
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.pstream_autograd(x, labels, s, tl, ll, blank, 0, 0.0, w)
    c2, g2 = pruned_ref.pruned_autograd(x, labels, s, tl, ll, blank, w)
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12) and np.allclose(g1, g2, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("seed", range(8))
def test_full_windows_are_the_materialised_references(seed, typ):
    """S = U with every start 0: tests/delay_ref.py (type 0, any penalty) and tests/mono_ref.py (type 1, penalty 0)."""
    from tests import delay_ref, mono_ref
    rng = np.random.default_rng(300 + seed)
    N, T, U, A = 4, int(rng.integers(3, 7)), int(rng.integers(1, 5)), 6
    case = dict(N=N, T=max(T, U - 1), U=U, S=U, type=typ)
    T = case["T"]
    tl, ll = F.lengths(case, rng)
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    x = rng.standard_normal((N, T, U, A))
    s = np.zeros((N, T), np.int32)
    blank, pen = int(rng.integers(0, A)), (0.4, -0.3)[seed % 2]
    if typ == 0:
        c1, g1 = R.pstream_autograd(x, labels, s, tl, ll, blank, 0, pen)
        c2, g2 = delay_ref.delay_autograd(x, labels, tl, ll, blank, pen)
    else:
        c1, g1 = R.pstream_autograd(x, labels, s, tl, ll, blank, 1, 0.0)
        c2, g2 = mono_ref.mono_autograd(x, labels, tl, ll, blank)
    assert np.isfinite(c1).all()
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12) and np.allclose(g1, g2, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("seed", range(6))
def test_the_k2_mapping(seed, typ):
    """px / py built from the pruned logits the way k2's get_rnnt_logprobs_pruned is documented to, the penalty added to px:
    minus the total of the px / py recursion (tests/mi_ref.py, the semantics of k2's mutual_information_recursion) is the
    reference's cost."""
    from tests import mi_ref
    for k in range(20):                                               # (the first problem of this seed's family with a label axis)
        x, labels, s, tl, ll, blank, penalty, S, _ = _tiny(seed + 40 * k, typ)
        if labels.shape[1] > 0:
            break
    assert labels.shape[1] > 0
    px, py, boundary = R.k2_px_py(x, labels, s, tl, ll, blank, typ, penalty)
    scores = mi_ref.mi_autograd(px, py, boundary)[0]
    c, _ = R.pstream_autograd(x, labels, s, tl, ll, blank, typ, penalty)
    assert np.isfinite(c).all() and np.allclose(-scores, c, rtol=1e-10, atol=1e-10), (scores, c)


# ----------------------------------------------------------------------------- the generators
def test_has_path_on_hand_made_windows():
    assert R.has_path([0, 0, 1], 3, 2, 2, 0) and R.has_path([0, 0, 1], 3, 2, 2, 1)
    assert R.has_path([0], 1, 1, 2, 0) and R.has_path([0], 1, 1, 1, 1) and not R.has_path([0], 1, 1, 1, 0)
    assert not R.has_path([0, 0], 2, 3, 4, 1) and R.has_path([0, 0], 2, 3, 4, 0)       # T_b < L_b
    assert not R.has_path([0, 1, 0], 3, 1, 1, 1)                                      # the last window misses (2, 1)
    assert R.max_labels(4, 1, 0) == 0 and R.max_labels(4, 3, 0) == 8 and R.max_labels(4, 3, 1) == 4


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_the_tables_generators(name):
    case = F.CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = F.lengths(case, rng)
    N, T, U, S, typ = case["N"], case["T"], case["U"], case["S"], case["type"]
    assert tl[0] == T and (tl >= 1).all() and (tl <= T).all() and (ll >= 0).all() and (ll < U).all()
    assert ll[0] == U - 1 or (typ == 0 and S == 1 and ll[0] == 0)
    if N >= 5:
        assert tl[1] == 1 and ll[2] == 0 and tl[F.FRAME_ZERO] == 1
        assert U == 1 or (typ == 0 and S == 1) or ll[F.FRAME_ZERO] >= 1
    if typ == 1:
        assert (ll <= tl).all()
    s = F.ranges(case, tl, ll, rng)
    assert s.shape == (N, T) and s.dtype == np.int32
    for b in range(N):
        Tb, Lb = int(tl[b]), int(ll[b])
        assert (s[b, :Tb] >= 0).all() and (s[b, :Tb] <= max(0, Lb + 1 - S)).all() and not s[b, Tb:].any()
        assert R.has_path(s[b], Tb, Lb, S, typ), (name, b)
    if case.get("burst") and typ == 0:
        assert (np.diff(s[0, :tl[0]]) == S - 1).any()
    if typ == 1 and S >= 2 and U >= 3:
        # a window partly outside the band: an in-lattice row the modified type never reads
        assert (R.in_lattice_mask((N, T, S), s, tl, ll) & ~R.read_mask((N, T, S), s, tl, ll, 1)).any(), name


def test_the_table_holds_the_listed_shapes():
    cs = F.CASES.values()
    for typ in (0, 1):
        mine = [c for c in cs if c["type"] == typ]
        assert {c["U"] for c in mine} >= {1, 2, 64, 65, 66, 130, 1100}
        assert {c["S"] for c in mine} >= {1, 2} and any(c["S"] == c["U"] > 2 for c in mine)
        assert any(c["S"] == 5 and c["U"] == 21 for c in mine) and any(c.get("burst") for c in mine)
        for d in ("f32", "f64"):
            wave = [c for c in mine if c["dtype"] == d and c["U"] <= 64]
            if typ:
                assert {c["T"] for c in wave} >= {F.MONO_CHUNK - 1, F.MONO_CHUNK, F.MONO_CHUNK + 1, 3 * F.MONO_CHUNK, 3 * F.MONO_CHUNK + 1}
            else:
                assert {c["T"] + c["U"] for c in wave} >= {F.AR_CHUNK - 1, F.AR_CHUNK, F.AR_CHUNK + 1, 3 * F.AR_CHUNK, 3 * F.AR_CHUNK + 1}
        assert any(c["dtype"] == "bf16" and c["U"] == 65 for c in mine) and any(c["dtype"] == "f16" and c["U"] == 65 for c in mine)
    for d, (_, _, _, esz) in F.STORES.items():
        assert {c["A"] for c in cs if c["dtype"] == d} >= {256 // esz, 256 // esz + 1, 2048 // esz, 2048 // esz + 1}
        assert any(c["dtype"] == d and c.get("off") == esz for c in cs)
    assert {c["A"] for c in cs} >= {3, 4, 5, 6, 7}
    assert all(c["N"] >= 5 for n, c in F.CASES.items() if "u1100" not in n)


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared
    for banned in ("mono", "delay", "hat", "mblank", "_ar", "_mi", "_kd"):
        assert not any(banned in s for s in declared), banned


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in ("libwarprnnt.so", "libwarprnnt_pruned.so", "libwarprnnt_mono.so", "libwarprnnt_delay.so", "libwarprnnt_mi.so"):
        got = I.exports(os.path.join(I.LIBDIR, lib))
        assert got and not any("pstream" in s for s in got), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import pstream
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(pstream.EXPORTS, HEADER) == []
    # the parameter lists are those of compute_rnnt_loss_pruned*, with rnnt_type (int) and delay_penalty (float) behind S;
    # the backward call takes neither; the workspace query takes S behind maxU
    pruned = I.declared_signatures("rnnt_pruned.h")
    for name, at in (("compute_rnnt_loss_pstream", 3), ("compute_rnnt_loss_pstream_fwd", 2)):
        sig = sigs[name]
        assert sig[at:at + 3] == ["int", "int", "float"], name
        assert sig[:at + 1] + sig[at + 3:] == pruned[name.replace("_pstream", "_pruned")], name
    assert sigs["compute_rnnt_loss_pstream_bwd"] == pruned["compute_rnnt_loss_pruned_bwd"]
    q = pruned["get_workspace_size_pruned"]
    assert sigs["get_workspace_size_pstream"] == q[:2] + ["int"] + q[2:]


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for g in (4, 16, 64):
        for tag in ("F32", "F64", "BF16", "F16"):
            assert "rnnt::pstream_stats_kernel<rnnt::%s, %d>" % (tag, g) in ks
    for tag in ("F32", "F64", "BF16", "F16"):
        assert "rnnt::mblank_grad_kernel<rnnt::%s>" % tag in ks and "rnnt::mblank_grad_elem_kernel<rnnt::%s>" % tag in ks
    for obj, lat in (("f32", "float"), ("f64", "double"), ("h16", "float")):
        for stage in ("prep", "close", "coef"):
            assert (obj, "rnnt::pstream_%s_kernel<%s>" % (stage, lat)) in rows
        for lattice in ("ar", "mono"):
            for form in ("wave", "block"):
                assert (obj, "rnnt::%s_lattice_%s_kernel<%s>" % (lattice, form, lat)) in rows


def test_the_tables_constants_are_the_kernels():
    csrc = os.path.join(ROOT, "warp-transducer_amd", "csrc")
    text = open(os.path.join(csrc, "rnnt_ar_kernels.h")).read()
    assert "constexpr int kArChunk = %d;" % F.AR_CHUNK in text and "constexpr int kArWaveMaxU = %d;" % F.AR_WAVE_MAX_U in text
    text = open(os.path.join(csrc, "rnnt_mono_kernels.h")).read()
    assert "constexpr int kMonoChunk = %d;" % F.MONO_CHUNK in text
    assert "constexpr int kMonoWaveMaxU = %d;" % F.MONO_WAVE_MAX_U in text


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
    for path, pattern in (("setup.py", '("pstream",)'), (mk, "SIDE += mi\nSIDE += pstream\n"),
                          (mk, "build/asan/test_pstream_args"), (mk, "delay mi pstream,$(SIDE))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS pstream)"), ("MANIFEST.in", "exports_pstream.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "exports_pstream.map"))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_pstream_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_pstream_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_pstream_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_pstream_args" in mk
    assert "build/asan/test_pstream_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import pstream
    x = torch.zeros(1, 2, 2, 5)
    i32 = dict(dtype=torch.int32)
    args = (torch.ones(1, 1, **i32), torch.tensor([2], **i32), torch.tensor([1], **i32), torch.zeros(1, 2, **i32))
    with pytest.raises(ValueError) as e:
        pstream.rnnt_loss_pruned_stream(x, *args)
    assert str(e.value) == "the pruned streaming loss runs on the GPU only: logits are on cpu"
    for bad in ("constrained", "Regular", "", None, 1):
        with pytest.raises(ValueError, match="'regular' or 'modified'"):
            pstream.rnnt_loss_pruned_stream(x, *args, rnnt_type=bad)
        with pytest.raises(ValueError, match="'regular' or 'modified'"):
            pstream.PrunedStreamingRNNTLoss(rnnt_type=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="delay_penalty must be finite"):
            pstream.PrunedStreamingRNNTLoss(delay_penalty=bad)
        with pytest.raises(ValueError, match="delay_penalty must be finite"):
            pstream.rnnt_loss_pruned_stream(x, *args, delay_penalty=bad)
    with pytest.raises(ValueError):
        pstream.PrunedStreamingRNNTLoss(reduction="max")
    with pytest.raises(ValueError):
        pstream.rnnt_loss_pruned_stream(x, *args, reduction="max")
    m = pstream.PrunedStreamingRNNTLoss(blank=3, rnnt_type="modified", delay_penalty=-0.5, reduction="sum", validate=False)
    assert (m.blank, m.rnnt_type, m.delay_penalty, m.reduction, m.validate) == (3, "modified", -0.5, "sum", False)
    assert pstream.type_code("regular") == 0 and pstream.type_code("modified") == 1
    import warprnnt_pytorch
    assert not hasattr(warprnnt_pytorch, "rnnt_loss_pruned_stream")     # a submodule: the package exports no side module
