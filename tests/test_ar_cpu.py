"""No GPU: the alignment-restricted loss's fp64 reference (tests/ar_ref.py) against brute-force path enumeration, closed
forms, the existing fp64 oracle under unrestricted windows, the band of include/rnnt_ar.h and its gradient formula;
libwarprnnt_ar.so's C-ABI and code objects against include/rnnt_ar.h and tests/ar_forms.py; and the refusals of
warprnnt_pytorch.ar that need no device."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import ar_forms as F
from tests import ar_ref as R
from tests import inventory as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_ar.so", "rnnt_ar.h"


def _tiny(seed, N=5):
    """Lattices up to T = 6, L = 4.  Sample 0 full, sample 1 with T_b = 1, sample 2 with L_b = 0, sample 3 fully pinned (one
    path), sample 4 unrestricted; feasible windows throughout."""
    rng = np.random.default_rng(7000 + seed)
    T, U, A = int(rng.integers(2, 7)), int(rng.integers(1, 6)), int(rng.integers(3, 8))
    case = dict(N=N, T=T, U=U)
    tl, ll = F.lengths(case, rng)
    lo, hi = F.windows(case, tl, ll, rng)
    blank = (0, A - 1, A // 2)[seed % 3]
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]        # (a label may equal the blank)
    x = rng.standard_normal((N, T, U, A)) * 1.5
    return x, labels, tl, ll, lo, hi, blank, rng


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_brute_force(seed):
    x, labels, tl, ll, lo, hi, blank, rng = _tiny(seed)
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.ar_autograd(x, labels, tl, ll, lo, hi, blank, w)
    c2, g2 = R.ar_brute(x, labels, tl, ll, lo, hi, blank, w)
    assert np.isfinite(c1).all()
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    # exact zeros outside the band, and the band is what enumeration walks through
    band = R.band_mask(x.shape, tl, ll, lo, hi)
    assert not g1[~band].any() and not g2[~band].any() and g1[band].any()
    for b in range(len(tl)):
        assert np.array_equal(R.paths_through(tl[b], ll[b], lo[b], hi[b]), band[b, :tl[b], :ll[b] + 1]), b
    assert not (band & ~R.in_lattice_mask(x.shape, tl, ll)).any()
    # whatever stands outside the band changes nothing, bit for bit
    xn = x.copy()
    xn[~band] = rng.standard_normal(int((~band).sum()) * x.shape[3]).reshape(-1, x.shape[3]) * 10
    c3, g3 = R.ar_autograd(xn, labels, tl, ll, lo, hi, blank, w)
    assert np.array_equal(c1, c3) and np.array_equal(g1, g3)


@pytest.mark.parametrize("seed", range(60))
def test_band_and_feasibility_statements_against_enumeration(seed):
    """Random windows, feasible or not: a path exists iff e_{u+1} <= l_u for every u, and then node (t, u) lies on one iff
    e_u <= t <= l_u."""
    rng = np.random.default_rng(900 + seed)
    for _ in range(25):
        T, L = int(rng.integers(1, 7)), int(rng.integers(0, 5))
        lo = rng.integers(-2, T + 2, size=L)
        hi = lo + rng.integers(-1, 4, size=L)
        e, l, ok = R.bounds(T, L, lo, hi)
        seen = R.paths_through(T, L, lo, hi)
        assert ok == bool(seen.any()), (T, L, lo, hi)
        band = R.band_mask((1, T, L + 1), [T], [L], [lo], [hi])[0]
        assert np.array_equal(band, seen), (T, L, lo, hi)


def test_the_weaker_condition_is_not_sufficient():
    """An empty window, lo_0 = 2 > hi_0 = 1 at T = 4: e = (0, 2) and l = (1, 3), so e_u <= l_u holds for every u, but
    e_1 = 2 > l_0 = 1 -- the header's statement -- and enumeration finds no path."""
    e, l, ok = R.bounds(4, 1, [2], [1])
    assert list(e) == [0, 2] and list(l) == [1, 3] and all(e[u] <= l[u] for u in range(2)) and not ok
    assert not R.paths_through(4, 1, [2], [1]).any()
    # windows that cannot be ordered: label 0 not before frame 2, label 1 not after frame 1
    e, l, ok = R.bounds(4, 2, [2, 0], [3, 1])
    assert not ok and not R.paths_through(4, 2, [2, 0], [3, 1]).any()


@pytest.mark.parametrize("seed", range(6))
def test_unrestricted_windows_are_the_oracles_rnnt(seed):
    from oracle import oracle as O
    x, labels, tl, ll, lo, hi, blank, _ = _tiny(seed)
    if x.shape[2] == 1:
        labels = np.zeros((x.shape[0], 0), np.int32)
    labels[labels == blank] = (blank + 1) % x.shape[3]        # (the oracle's lattice has no label on the blank column)
    lo, hi = np.full_like(lo, -5), np.full_like(hi, 99)
    lo[0, :] = 0                                          # lo = 0, hi = T_b - 1: the tightest "unrestricted"
    hi[0, :] = tl[0] - 1
    c1, g1 = R.ar_autograd(x, labels, tl, ll, lo, hi, blank)
    c2, g2 = O.rnnt_logits(x, labels, tl, ll, blank)
    assert np.allclose(c1, c2, rtol=1e-10, atol=0)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    assert np.array_equal(R.band_mask(x.shape, tl, ll, lo, hi), R.in_lattice_mask(x.shape, tl, ll))


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_fully_pinned(seed):
    """Every label pinned to its frame: one path, cost = -(the labels at their frames + the blanks between them)."""
    rng = np.random.default_rng(seed)
    T, L, A, blank = int(rng.integers(2, 7)), int(rng.integers(1, 5)), 6, seed % 6
    x = rng.standard_normal((1, T, L + 1, A))
    labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
    a = np.sort(rng.integers(0, T, size=L))
    lp = torch.log_softmax(torch.tensor(x[0]), -1).numpy()
    want, u = 0.0, 0
    for t in range(T):
        while u < L and a[u] == t:
            want += lp[t, u, labels[0, u]]
            u += 1
        want += lp[t, u, blank]
    for fn in (R.ar_autograd, R.ar_brute):
        c, g = fn(x, labels, [T], [L], [a], [a], blank)
        assert abs(c[0] + want) < 1e-12, (fn, c, want)
    assert int(R.band_mask(x.shape, [T], [L], [a], [a]).sum()) == T + L


@pytest.mark.parametrize("seed", range(8))
def test_gradient_formula_of_the_header(seed):
    x, labels, tl, ll, lo, hi, blank, _ = _tiny(seed)
    if seed % 2 and labels.size:
        labels[0, 0] = blank                         # a label that equals the blank: both posteriors in one column
    _, g = R.ar_autograd(x, labels, tl, ll, lo, hi, blank)
    assert np.allclose(R.ar_formula(x, labels, tl, ll, lo, hi, blank), g, rtol=1e-12, atol=1e-14)


def test_infeasible_windows_cost_infinity():
    """An empty window, lo_0 > hi_1, and a window wholly past T_b; a healthy sample beside them."""
    rng = np.random.default_rng(9)
    x = rng.standard_normal((4, 5, 3, 5))
    labels = rng.integers(0, 5, size=(4, 2)).astype(np.int32)
    tl, ll = np.array([5, 5, 3, 5], np.int32), np.array([2, 2, 2, 2], np.int32)
    lo = np.array([[2, 0], [3, 0], [0, 3], [1, 2]], np.int32)
    hi = np.array([[1, 4], [4, 2], [4, 9], [2, 3]], np.int32)
    for fn in (R.ar_autograd, R.ar_brute):
        c, g = fn(x, labels, tl, ll, lo, hi, 0)
        assert np.isposinf(c[:3]).all() and np.isfinite(c[3]) and not g[:3].any() and g[3].any()
    band = R.band_mask(x.shape, tl, ll, lo, hi)
    assert not band[:3].any() and band[3].any()
    assert [R.bounds(tl[b], ll[b], lo[b], hi[b])[2] for b in range(4)] == [False, False, False, True]


def test_the_tables_generators():
    """Every case's batch: the full sample, T_b = 1, L_b = 0, a pinned sample with a single path and an unrestricted one; all
    feasible."""
    for name, case in F.CASES.items():
        rng = np.random.default_rng(1)
        tl, ll = F.lengths(case, rng)
        lo, hi = F.windows(case, tl, ll, rng)
        N, T, U = case["N"], case["T"], case["U"]
        assert tl[0] == T and ll[0] == U - 1 and tl[1] == 1 and (tl >= 1).all() and (tl <= T).all() and (ll < U).all(), name
        assert lo.shape == hi.shape == (N, U - 1) and lo.dtype == hi.dtype == np.int32
        band = R.band_mask((N, T, U), tl, ll, lo, hi)
        assert all(R.bounds(tl[b], ll[b], lo[b], hi[b])[2] for b in range(N)) and band.any(-1).any(-1).all(), name
        if N >= 5:
            assert ll[2] == 0, name
            if U > 1:
                p, q = F.PINNED, F.UNRESTRICTED
                assert ll[p] >= 1 and int(band[p].sum()) == tl[p] + ll[p], name          # a single path
                assert ll[q] >= 1 and np.array_equal(band[q], R.in_lattice_mask((N, T, U), tl, ll)[q]), name


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_exports_unchanged():
    """The other side libraries export exactly their headers, and neither they nor the main library anything of this one."""
    I.need_lib(LIB)
    for lib, header in (("libwarprnnt_tdt.so", "rnnt_tdt.h"), ("libwarprnnt_pruned.so", "rnnt_pruned.h"),
                        ("libwarprnnt_hat.so", "rnnt_hat.h"), ("libwarprnnt_mblank.so", "rnnt_mblank.h"),
                        ("libwarprnnt_tdt_align.so", "rnnt_tdt_align.h"), ("libwarprnnt_mono.so", "rnnt_mono.h")):
        got = I.exports(os.path.join(I.LIBDIR, lib))
        assert got == I.declared(header) and not any(s.endswith("_ar") or "_ar_" in s for s in got), lib
    main = I.exports(os.path.join(I.LIBDIR, "libwarprnnt.so"))
    assert "compute_rnnt_loss" in main and not any(s.endswith("_ar") or "_ar_" in s for s in main)
    from warprnnt_pytorch import _lib
    assert {s for s in main if not s.startswith("_")} >= set(_lib.EXPORTS)


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import ar
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(ar.EXPORTS, HEADER) == []
    # the parameter lists are those of compute_rnnt_loss_mono*, two pointers (the windows) behind input_lengths: the fifth
    # parameter of the one-call entry, the fourth of _fwd
    mono = I.declared_signatures("rnnt_mono.h")
    behind = {"compute_rnnt_loss_ar": 5, "compute_rnnt_loss_ar_fwd": 4}
    for name, sig in sigs.items():
        at = behind.get(name)
        if at is not None:
            assert sig[at:at + 2] == ["pointer", "pointer"], name
            sig = sig[:at] + sig[at + 2:]
        assert sig == mono[name.replace("_ar", "_mono")], name
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert text.count("const int* input_lengths, const int* emit_lo,") == 2 and text.count("const int* emit_hi") == 2


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for g in (4, 16, 64):
        for tag in ("F32", "F64", "BF16", "F16"):
            assert "rnnt::ar_stats_kernel<rnnt::%s, %d>" % (tag, g) in ks
    for obj, lat in (("f32", "float"), ("f64", "double"), ("h16", "float")):
        assert (obj, "rnnt::ar_bounds_kernel<%s>" % lat) in rows
        for form in ("wave", "block"):
            assert (obj, "rnnt::ar_lattice_%s_kernel<%s>" % (form, lat)) in rows
    assert {c["U"] for c in F.CASES.values()} >= {1, 2, F.WAVE_MAX_U, F.WAVE_MAX_U + 1, 130, 1100}
    steps = {c["T"] + c["U"] - 1 for c in F.CASES.values()}
    assert steps >= {F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 3 * F.CHUNK}


def test_the_tables_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_ar_kernels.h")).read()
    assert "constexpr int kArChunk = %d;" % F.CHUNK in text and "constexpr int kArWaveMaxU = %d;" % F.WAVE_MAX_U in text


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
def test_check_windows_names_the_first_label_without_a_frame():
    """validate=True: the sample and the label are named, with e_{u+1} and l_u.  (Host arithmetic: it needs no device.)"""
    from warprnnt_pytorch import ar
    i32 = dict(dtype=torch.int32)
    tl, ll = torch.tensor([5, 5, 3], **i32), torch.tensor([2, 2, 1], **i32)
    lo, hi = torch.tensor([[1, 2], [3, 0], [0, -1]], **i32), torch.tensor([[2, 3], [4, 2], [9, -1]], **i32)
    with pytest.raises(ValueError) as e:
        ar.check_windows(tl, ll, lo, hi)
    assert str(e.value) == "sample 1 has no path: label 0 needs a frame in [3, 2]"
    hi[1, 1] = 3
    ar.check_windows(tl, ll, lo, hi)
    lo[2, 0] = 3                                            # wholly past T_2 = 3
    with pytest.raises(ValueError, match=r"sample 2 has no path: label 0 needs a frame in \[3, 2\]"):
        ar.check_windows(tl, ll, lo, hi)
    lo[2, 0], lo[0, 1], hi[0, 1] = 0, 4, 3                  # an empty window
    with pytest.raises(ValueError, match=r"sample 0 has no path: label 1 needs a frame in \[4, 3\]"):
        ar.check_windows(tl, ll, lo, hi)
    # the message's numbers are the reference's e_{u+1} and l_u
    e, l, ok = R.bounds(5, 2, lo[0].numpy(), hi[0].numpy())
    assert not ok and (e[2], l[1]) == (4, 3)


def test_alignment_windows():
    from warprnnt_pytorch import ar
    frames = torch.tensor([[0, 3, 7], [2, -1, -1]], dtype=torch.int32)
    lo, hi = ar.alignment_windows(frames, 2, 5)
    assert lo.dtype == hi.dtype == torch.int32 and lo.device == frames.device
    assert lo.tolist() == [[-2, 1, 5], [0, -1, -1]] and hi.tolist() == [[5, 8, 12], [7, -1, -1]]
    lo, hi = ar.alignment_windows(frames, torch.tensor([0, 1, 2]), torch.tensor([[3], [0]]))
    assert lo.tolist() == [[0, 2, 5], [2, -1, -1]] and hi.tolist() == [[3, 6, 10], [2, -1, -1]]
    lo, hi = ar.alignment_windows(frames, 0, 0)
    assert torch.equal(lo, frames) and torch.equal(hi, frames)


def test_python_refuses_cpu_tensors_dtypes_and_bad_reductions():
    from warprnnt_pytorch import ar
    x = torch.zeros(1, 2, 2, 5)
    i32 = dict(dtype=torch.int32)
    args = (torch.ones(1, 1, **i32), torch.tensor([2], **i32), torch.tensor([1], **i32), torch.zeros(1, 1, **i32),
            torch.ones(1, 1, **i32))
    with pytest.raises(ValueError) as e:
        ar.rnnt_loss_ar(x, *args)
    assert "GPU" in str(e.value) and str(e.value) == "the alignment-restricted loss runs on the GPU only: logits are on cpu"
    with pytest.raises(ValueError):
        ar.AlignmentRestrictedRNNTLoss(reduction="max")
    with pytest.raises(ValueError):
        ar.rnnt_loss_ar(x, *args, reduction="max")
    with pytest.raises(TypeError, match="labels must be torch.int32"):
        ar.rnnt_loss_ar(x, args[0].long(), *args[1:])
    with pytest.raises(TypeError, match="emit_lo must be torch.int32"):
        ar.rnnt_loss_ar(x, *args[:3], args[3].long(), args[4])
    with pytest.raises(TypeError, match="emit_hi must be torch.int32"):
        ar.rnnt_loss_ar(x, *args[:4], args[4].long())
