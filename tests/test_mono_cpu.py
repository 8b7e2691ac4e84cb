"""No GPU: the monotonic loss's fp64 reference (tests/mono_ref.py) against brute-force path enumeration, closed forms, the
existing fp64 oracle at L_b = 0, the band of include/rnnt_mono.h and its gradient formula; libwarprnnt_mono.so's C-ABI and
code objects against include/rnnt_mono.h and tests/mono_forms.py; and the refusals of warprnnt_pytorch.mono that need no
device."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import mono_forms as F
from tests import mono_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_mono.so", "rnnt_mono.h"


def _tiny(seed, N=5):
    """Lattices up to T = 6, L = 4, every T_b >= L_b.  Sample 0 full, sample 1 with T_b = L_b (one path), sample 2 with
    L_b = 0, sample 3 with T_b = 1, sample 4 with T_b = L_b + 1."""
    rng = np.random.default_rng(5000 + seed)
    T, U, A = int(rng.integers(3, 7)), int(rng.integers(1, 6)), int(rng.integers(3, 8))
    U = min(U, T + 1)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl = np.array([rng.integers(max(int(l), 1), T + 1) for l in ll]).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    ll[1] = max(U - 1, 0)
    tl[1] = max(ll[1], 1)
    ll[2] = 0
    tl[3], ll[3] = 1, min(seed % 2, U - 1)
    ll[4] = rng.integers(0, min(U - 1, T - 1) + 1)
    tl[4] = ll[4] + 1
    blank = (0, A - 1, A // 2)[seed % 3]
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]        # (a label may equal the blank)
    x = rng.standard_normal((N, T, U, A)) * 1.5
    return x, labels, tl, ll, blank, rng


def _band_rows(T, L):
    return (L + 1) * (T - L) + L


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_brute_force(seed):
    x, labels, tl, ll, blank, rng = _tiny(seed)
    assert (tl >= ll).all()
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.mono_autograd(x, labels, tl, ll, blank, w)
    c2, g2 = R.mono_brute(x, labels, tl, ll, blank, w)
    assert np.isfinite(c1).all()
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    # exact zeros outside the band, and the band holds (L + 1)(T - L) + L rows
    band = R.band_mask(x.shape, tl, ll)
    assert not g1[~band].any() and not g2[~band].any() and g1[band].any()
    assert [int(band[b].sum()) for b in range(len(tl))] == [_band_rows(int(t), int(l)) for t, l in zip(tl, ll)]
    assert not (band & ~R.in_lattice_mask(x.shape, tl, ll)).any()
    # whatever stands outside the band changes nothing, bit for bit
    xn = x.copy()
    xn[~band] = rng.standard_normal(int((~band).sum()) * x.shape[3]).reshape(-1, x.shape[3]) * 10
    c3, g3 = R.mono_autograd(xn, labels, tl, ll, blank, w)
    assert np.array_equal(c1, c3) and np.array_equal(g1, g3)


def test_no_path_with_fewer_frames_than_labels():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, 4, 4, 5))
    labels = rng.integers(0, 5, size=(2, 3)).astype(np.int32)
    tl, ll = np.array([2, 4], np.int32), np.array([3, 3], np.int32)
    for fn in (R.mono_autograd, R.mono_brute):
        c, g = fn(x, labels, tl, ll, 0)
        assert np.isposinf(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
    assert not R.band_mask(x.shape, tl, ll)[0].any()


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_single_path(seed):
    """T_b = L_b: the one path takes a label in every frame, cost = -sum_t lp(t, t, y_t)."""
    rng = np.random.default_rng(seed)
    L, A, blank = int(rng.integers(1, 6)), 6, seed % 6
    x = rng.standard_normal((1, L, L + 1, A))
    labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
    lp = torch.log_softmax(torch.tensor(x[0]), -1).numpy()
    want = -sum(lp[t, t, labels[0, t]] for t in range(L))
    for fn in (R.mono_autograd, R.mono_brute):
        c, _ = fn(x, labels, [L], [L], blank)
        assert abs(c[0] - want) < 1e-12, (fn, c, want)


@pytest.mark.parametrize("seed", range(6))
def test_against_the_oracles_plain_rnnt(seed):
    """L_b = 0: T_b blanks, the plain RNN-T cost.  L_b >= 1 and T_b > L_b: the two losses differ."""
    from oracle import oracle as O
    x, labels, tl, ll, blank, _ = _tiny(seed)
    if x.shape[2] == 1:
        labels = np.zeros((x.shape[0], 0), np.int32)
    c1, g1 = R.mono_autograd(x, labels, tl, ll, blank)
    c2, g2 = O.rnnt_logits(x, labels, tl, ll, blank)
    for b in range(len(tl)):
        if ll[b] == 0:
            assert abs(c1[b] - c2[b]) < 1e-12 * max(1.0, abs(c2[b]))
            assert np.allclose(g1[b], g2[b], rtol=1e-10, atol=1e-12)
        elif tl[b] > ll[b]:
            assert abs(c1[b] - c2[b]) > 1e-6, (b, c1, c2)


@pytest.mark.parametrize("seed", range(8))
def test_gradient_formula_of_the_header(seed):
    x, labels, tl, ll, blank, _ = _tiny(seed)
    if seed % 2 and labels.size:
        labels[0, 0] = blank                         # a label that equals the blank: both posteriors in one column
    _, g = R.mono_autograd(x, labels, tl, ll, blank)
    assert np.allclose(R.mono_formula(x, labels, tl, ll, blank), g, rtol=1e-12, atol=1e-14)


def test_the_tables_length_generator():
    """Every case's batch: T_b >= L_b throughout; the full sample, T_b = 1, L_b = 0, T_b = L_b and T_b = L_b + 1."""
    for name, case in F.CASES.items():
        tl, ll = F.lengths(case, np.random.default_rng(1))
        assert (tl >= ll).all() and tl[0] == case["T"] and ll[0] == min(case["U"] - 1, case["T"]) and tl[1] == 1, name
        if case["N"] >= 5:
            assert ll[2] == 0 and tl[4] == ll[4] + 1 and (case["U"] == 1 or tl[3] == ll[3]), name


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_exports_unchanged():
    """The other side libraries export exactly their headers, and neither they nor the main library anything of this one."""
    I.need_lib(LIB)
    for lib, header in (("libwarprnnt_tdt.so", "rnnt_tdt.h"), ("libwarprnnt_pruned.so", "rnnt_pruned.h"),
                        ("libwarprnnt_hat.so", "rnnt_hat.h"), ("libwarprnnt_mblank.so", "rnnt_mblank.h"),
                        ("libwarprnnt_tdt_align.so", "rnnt_tdt_align.h")):
        got = I.exports(os.path.join(I.LIBDIR, lib))
        assert got == I.declared(header) and not any("mono" in s for s in got), lib
    main = I.exports(os.path.join(I.LIBDIR, "libwarprnnt.so"))
    assert "compute_rnnt_loss" in main and not any("mono" in s for s in main)
    from warprnnt_pytorch import _lib
    assert {s for s in main if not s.startswith("_")} >= set(_lib.EXPORTS)


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import mono
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(mono.EXPORTS, HEADER) == []
    # the parameter lists are those of compute_hat_loss*
    hat = I.declared_signatures("rnnt_hat.h")
    assert {k.replace("compute_rnnt_loss_mono", "compute_hat_loss").replace("_mono", "_hat"): v for k, v in sigs.items()} == hat


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for g in (4, 16, 64):
        for tag in ("F32", "F64", "BF16", "F16"):
            assert "rnnt::mono_stats_kernel<rnnt::%s, %d>" % (tag, g) in ks
    # the corners of the shared row reduction (csrc/rnnt_row_lse.h), for every store and group size: rows off a 16-byte
    # boundary, and rows that take a second round of four packets per lane
    for d, (_, tag, _, esz) in F.STORES.items():
        for g in (4, 16, 64):
            got = [F.C.row_corners(esz, c["A"], g, c.get("off", 0)) for c in F.CASES.values()
                   if c["dtype"] == d and F.stats_group(c["A"] * esz) == g]
            assert any(skip for skip, _ in got) and any(rounds >= 2 for _, rounds in got), (d, g, got)
    for obj, lat in (("f32", "float"), ("f64", "double"), ("h16", "float")):
        for form in ("wave", "block"):
            assert (obj, "rnnt::mono_lattice_%s_kernel<%s>" % (form, lat)) in rows
    assert {c["U"] for c in F.CASES.values()} >= {1, 2, F.WAVE_MAX_U, F.WAVE_MAX_U + 1, 130, 1100}
    assert {c["T"] for c in F.CASES.values()} >= {F.CHUNK - 1, F.CHUNK, F.CHUNK + 1}


def test_the_tables_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_mono_kernels.h")).read()
    assert "constexpr int kMonoChunk = %d;" % F.CHUNK in text and "constexpr int kMonoWaveMaxU = %d;" % F.WAVE_MAX_U in text


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


# ----------------------------------------------------------------------------- the Python module, without a device
def test_python_refuses_fewer_frames_than_labels():
    """validate=True: the sample is named.  (The check rides behind the read-back of the lengths; it needs no device.)"""
    from warprnnt_pytorch import mono
    tl, ll = torch.tensor([5, 2, 4], dtype=torch.int32), torch.tensor([3, 3, 4], dtype=torch.int32)
    with pytest.raises(ValueError, match="sample 1 has 2 frames for 3 labels"):
        mono.check_paths(tl, ll)
    mono.check_paths(torch.tensor([5, 3, 4], dtype=torch.int32), ll)


def test_python_refuses_cpu_tensors_and_bad_reductions():
    from warprnnt_pytorch import mono
    x = torch.zeros(1, 2, 2, 5)
    args = (torch.ones(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))
    with pytest.raises(ValueError) as e:
        mono.rnnt_loss_mono(x, *args)
    assert str(e.value) == "the monotonic loss runs on the GPU only: logits are on cpu"
    with pytest.raises(ValueError):
        mono.MonotonicRNNTLoss(reduction="max")
    with pytest.raises(TypeError, match="labels must be torch.int32"):
        mono.rnnt_loss_mono(x, args[0].long(), *args[1:])
