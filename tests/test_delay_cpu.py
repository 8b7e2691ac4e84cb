"""No GPU: the delay-penalized loss's fp64 reference (tests/delay_ref.py) against brute-force path enumeration, the existing
fp64 oracle at a penalty of 0, the derivative identity of include/rnnt_delay.h and the range of the expected emission frames;
libwarprnnt_delay.so's C-ABI and code objects against include/rnnt_delay.h and tests/delay_forms.py; the build lists; and the
refusals of warprnnt_pytorch.delay that need no device."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import delay_forms as F
from tests import delay_ref as R
from tests import inventory as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_delay.so", "rnnt_delay.h"


def _tiny(seed, N=5, max_t=5, max_l=3):
    """Lattices up to T = max_t, L = max_l.  Sample 0 full, sample 1 with T_b = 1, sample 2 with L_b = 0, sample 3 with
    T_b = 1 and L_b >= 1."""
    rng = np.random.default_rng(8000 + seed)
    T, U, A = int(rng.integers(2, max_t + 1)), int(rng.integers(1, max_l + 2)), int(rng.integers(3, 8))
    tl, ll = F.lengths(dict(N=N, T=T, U=U), rng)
    blank = (0, A - 1, A // 2)[seed % 3]
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]        # (a label may equal the blank)
    x = rng.standard_normal((N, T, U, A)) * 1.5
    penalty = (0.3, -0.7, 0.05, 1.5)[seed % 4]
    return x, labels, tl, ll, blank, penalty, rng


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_brute_force(seed):
    x, labels, tl, ll, blank, penalty, rng = _tiny(seed)
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.delay_autograd(x, labels, tl, ll, blank, penalty, w)
    c2, g2 = R.delay_brute(x, labels, tl, ll, blank, penalty, w)
    assert np.isfinite(c1).all()
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    inl = R.in_lattice_mask(x.shape, tl, ll)
    assert not g1[~inl].any() and g1[inl].any()
    e1 = R.emit_frames_ref(x, labels, tl, ll, blank, penalty)
    e2 = R.emit_frames_brute(x, labels, tl, ll, blank, penalty)
    assert np.allclose(e1, e2, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("seed", range(8))
def test_penalty_zero_is_the_oracles_rnnt(seed):
    from oracle import oracle as O
    x, labels, tl, ll, blank, _, _ = _tiny(seed)
    if x.shape[2] == 1:
        labels = np.zeros((x.shape[0], 0), np.int32)
    labels[labels == blank] = (blank + 1) % x.shape[3]        # (the oracle's lattice has no label on the blank column)
    c1, g1 = R.delay_autograd(x, labels, tl, ll, blank, 0.0)
    c2, g2 = O.rnnt_logits(x, labels, tl, ll, blank)
    assert np.allclose(c1, c2, rtol=1e-10, atol=0)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("seed", range(12))
def test_derivative_identity(seed):
    """d cost_b / d delay_penalty = -sum_{u < L_b} ((T_b - 1) / 2 - emit_frames[b, u]), by central difference in fp64 with
    h = 1e-4 at T <= 6, L <= 3: truncation is at most h^2 / 6 (L T)^3 ~ 1e-5, rounding eps cost / h ~ 1e-11."""
    x, labels, tl, ll, blank, penalty, _ = _tiny(seed, max_t=6, max_l=3)
    h = 1e-4
    cp, _ = R.delay_autograd(x, labels, tl, ll, blank, penalty + h)
    cm, _ = R.delay_autograd(x, labels, tl, ll, blank, penalty - h)
    e = R.emit_frames_ref(x, labels, tl, ll, blank, penalty)
    want = np.array([-sum(0.5 * (tl[b] - 1) - e[b, u] for u in range(ll[b])) for b in range(len(tl))])
    assert np.abs((cp - cm) / (2 * h) - want).max() <= 1e-4, ((cp - cm) / (2 * h), want)


@pytest.mark.parametrize("seed", range(12))
def test_emit_frames_are_ordered_and_inside_the_utterance(seed):
    x, labels, tl, ll, blank, penalty, _ = _tiny(seed, max_t=7, max_l=4)
    e = R.emit_frames_ref(x, labels, tl, ll, blank, penalty)
    for b in range(len(tl)):
        row = e[b, :ll[b]]
        assert (row >= -1e-12).all() and (row <= tl[b] - 1 + 1e-12).all(), (b, row)
        assert (np.diff(row) >= -1e-12).all(), (b, row)
        assert not e[b, ll[b]:].any()
        if tl[b] == 1:
            assert not row.any()


def test_closed_form_single_frame():
    """T_b = 1: every label at frame 0, one path, cost = -(sum of its log-probabilities) - delay_penalty * L * 0."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 1, 4, 6))
    labels = rng.integers(0, 6, size=(1, 3)).astype(np.int32)
    lp = torch.log_softmax(torch.tensor(x[0, 0]), -1).numpy()
    want = -(sum(lp[u, labels[0, u]] for u in range(3)) + lp[3, 2])
    for pen in (0.0, 0.9, -2.0):
        c, _ = R.delay_autograd(x, labels, [1], [3], 2, pen)
        assert abs(c[0] - want) < 1e-12
        assert not R.emit_frames_ref(x, labels, [1], [3], 2, pen).any()


def test_the_tables_generators():
    for name, case in F.CASES.items():
        rng = np.random.default_rng(1)
        tl, ll = F.lengths(case, rng)
        N, T, U = case["N"], case["T"], case["U"]
        assert tl[0] == T and ll[0] == U - 1 and (tl >= 1).all() and (tl <= T).all() and (ll >= 0).all() and (ll < U).all(), name
        if N >= 5:
            assert tl[1] == 1 and ll[2] == 0 and tl[F.FRAME_ZERO] == 1, name
            assert U == 1 or ll[F.FRAME_ZERO] >= 1, name


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in ("libwarprnnt.so", "libwarprnnt_ar.so", "libwarprnnt_mono.so", "libwarprnnt_mblank.so", "libwarprnnt_kd.so"):
        got = I.exports(os.path.join(I.LIBDIR, lib))
        assert got and not any("delay" in s for s in got), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import delay
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(delay.EXPORTS, HEADER) == []
    # the parameter lists are those of compute_rnnt_loss_mono*: the penalty, a float, behind the activations and the
    # emit_frames pointer behind the costs
    mono = I.declared_signatures("rnnt_mono.h")
    emit_at = {"compute_rnnt_loss_delay": 9, "compute_rnnt_loss_delay_fwd": 8}
    for name, sig in sigs.items():
        at = emit_at.get(name)
        if at is not None:
            assert sig[1] == "float" and sig[at] == "pointer", name
            sig = [k for i, k in enumerate(sig) if i not in (1, at)]
        assert sig == mono[name.replace("_delay", "_mono")], name


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for g in (4, 16, 64):
        for tag in ("F32", "F64", "BF16", "F16"):
            assert "rnnt::delay_stats_kernel<rnnt::%s, %d>" % (tag, g) in ks
    for obj, lat in (("f32", "float"), ("f64", "double"), ("h16", "float")):
        assert (obj, "rnnt::delay_coef_kernel<%s>" % lat) in rows
        for form in ("wave", "block"):
            assert (obj, "rnnt::ar_lattice_%s_kernel<%s>" % (form, lat)) in rows
        for s in (1, F.EMIT_SLICES):
            assert (obj, "rnnt::delay_emit_kernel<%s, %d>" % (lat, s)) in rows
    us = {c["U"] for c in F.CASES.values()}
    assert us >= {1, 2, F.WAVE_MAX_U, F.WAVE_MAX_U + 1, 130, 1100}
    # the emission kernel's rule and its blocks: 32 | 33 and 64 | 65 and 256 | 257 label columns
    assert us >= {33, 34, F.EMIT_NARROW + 1, F.EMIT_NARROW + 2, 257, 258}
    steps = {c["T"] + c["U"] - 1 for c in F.CASES.values()}
    assert steps >= {F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 3 * F.CHUNK}
    assert F.predict(F.CASES["f32_u1"], 256)["emit"] == set()


def test_the_tables_constants_are_the_kernels():
    csrc = os.path.join(ROOT, "warp-transducer_amd", "csrc")
    text = open(os.path.join(csrc, "rnnt_ar_kernels.h")).read()
    assert "constexpr int kArChunk = %d;" % F.CHUNK in text and "constexpr int kArWaveMaxU = %d;" % F.WAVE_MAX_U in text
    text = open(os.path.join(csrc, "rnnt_delay_kernels.h")).read()
    assert "constexpr int kDelayEmitSlices = %d;" % F.EMIT_SLICES in text
    assert "constexpr int kDelayEmitNarrow = %d;" % F.EMIT_NARROW in text


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
    for path, pattern in (("setup.py", '"kd", "delay")'), (os.path.join("warp-transducer_amd", "Makefile"), " kd delay\n"),
                          ("CMakeLists.txt", " kd delay)"), ("MANIFEST.in", "exports_delay.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), path
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "exports_delay.map"))


# ----------------------------------------------------------------------------- the Python module, without a device
def test_python_refuses_cpu_tensors_dtypes_bad_reductions_and_penalties():
    from warprnnt_pytorch import delay
    x = torch.zeros(1, 2, 2, 5)
    i32 = dict(dtype=torch.int32)
    args = (torch.ones(1, 1, **i32), torch.tensor([2], **i32), torch.tensor([1], **i32))
    with pytest.raises(ValueError) as e:
        delay.rnnt_loss_delay(x, *args)
    assert str(e.value) == "the delay-penalized loss runs on the GPU only: logits are on cpu"
    with pytest.raises(ValueError, match="GPU"):
        delay.expected_emit_frames(x, *args)
    with pytest.raises(ValueError):
        delay.DelayPenalizedRNNTLoss(reduction="max")
    with pytest.raises(ValueError):
        delay.rnnt_loss_delay(x, *args, reduction="max")
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="delay_penalty must be finite"):
            delay.DelayPenalizedRNNTLoss(delay_penalty=bad)
    with pytest.raises(TypeError, match="labels must be torch.int32"):
        delay.rnnt_loss_delay(x, args[0].long(), *args[1:])
    import warprnnt_pytorch
    assert not hasattr(warprnnt_pytorch, "rnnt_loss_delay")          # a submodule: the package exports no side module
