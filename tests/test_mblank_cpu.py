"""No GPU: the multi-blank loss's fp64 reference (tests/mblank_ref.py) against brute-force path enumeration, the existing fp64
oracle at K = 0, a closed form and the gradient formula of include/rnnt_mblank.h; and libwarprnnt_mblank.so's C-ABI and code
objects against include/rnnt_mblank.h and tests/mblank_forms.py."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import mblank_forms as F
from tests import mblank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_mblank.so", "rnnt_mblank.h"
DURS = (2, 3)


def _tiny(seed, N=4):
    """Lattices up to T = 5, L = 3 with durations (2, 3).  Sample 0 full, sample 1 with L_b = 0, sample 2 with T_b = 1 (every
    big blank overshoots), sample 3 with L_b = 0 and T_b a duration (a big blank enters the terminal node from (0, 0))."""
    rng = np.random.default_rng(3000 + seed)
    T, U, A = int(rng.integers(3, 6)), int(rng.integers(1, 5)), int(rng.integers(4, 8))
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    ll[1] = 0
    tl[2] = 1
    tl[3], ll[3] = DURS[seed % 2], 0
    blank = (0, A - 1, A // 2)[seed % 3]
    others = [c for c in range(A) if c != blank]
    cols = tuple(int(c) for c in rng.permutation(others)[:2])
    allowed = [c for c in others if c not in cols]
    labels = rng.choice(allowed, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    x = rng.standard_normal((N, T, U, A)) * 1.5
    sigma = 0.05 if seed % 4 == 0 else 0.0
    return x, labels, tl, ll, cols, blank, sigma, rng


@pytest.mark.parametrize("seed", range(40))
def test_reference_equals_brute_force(seed):
    x, labels, tl, ll, cols, blank, sigma, rng = _tiny(seed)
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.mblank_autograd(x, labels, tl, ll, cols, DURS, blank, sigma, w)
    c2, g2 = R.mblank_brute(x, labels, tl, ll, cols, DURS, blank, sigma, w)
    assert np.isfinite(c1).all()
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    mask = R.in_lattice_mask(x.shape, tl, ll)
    assert not g1[~mask].any() and g1[mask].any()
    # T_b = 1: no big blank fits, the big-blank columns get the softmax term alone (a plain RNN-T row)
    c0, g0 = R.mblank_autograd(x[2:3], labels[2:3], tl[2:3], ll[2:3], (), (), blank, sigma, w[2:3])
    assert abs(c0[0] - c1[2]) < 1e-12 and np.allclose(g0[0], g1[2], rtol=1e-12, atol=1e-14)


def test_big_blanks_change_the_loss():
    x, labels, tl, ll, cols, blank, sigma, _ = _tiny(1)
    c1, _ = R.mblank_autograd(x, labels, tl, ll, cols, DURS, blank, sigma)
    c0, _ = R.mblank_autograd(x, labels, tl, ll, (), (), blank, sigma)
    assert c1[0] < c0[0] - 1e-3 and c1[3] < c0[3] - 1e-3          # (more paths: a smaller cost)


@pytest.mark.parametrize("seed", range(6))
def test_without_big_blanks_it_is_the_oracles_rnnt(seed):
    x, labels, tl, ll, _, blank, _, _ = _tiny(seed)
    from oracle import oracle as O
    if x.shape[2] == 1:
        labels = np.zeros((x.shape[0], 0), np.int32)
    c1, g1 = R.mblank_autograd(x, labels, tl, ll, (), (), blank, 0.0)
    c2, g2 = O.rnnt_logits(x, labels, tl, ll, blank)
    mask = R.in_lattice_mask(x.shape, tl, ll)
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1[mask], g2[mask], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("seed", range(8))
def test_gradient_formula_of_the_header(seed):
    x, labels, tl, ll, cols, blank, sigma, _ = _tiny(seed)
    if seed % 2 and labels.size:
        labels[0, 0] = cols[0]                       # a label that equals a big-blank column: both posteriors in one column
        if labels.shape[1] > 1:
            labels[0, 1] = blank
    _, g = R.mblank_autograd(x, labels, tl, ll, cols, DURS, blank, sigma)
    assert np.allclose(R.mblank_formula(x, labels, tl, ll, cols, DURS, blank, sigma), g, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("d", [2, 3, 5])
def test_closed_form_two_paths(d):
    """T = d, L = 0, K = 1: exactly two paths -- d standard blanks, or one big blank."""
    rng = np.random.default_rng(d)
    A, blank, col = 5, 1, 3
    x = rng.standard_normal((1, d, 1, A))
    for sigma in (0.0, 0.05):
        lp = torch.log_softmax(torch.tensor(x[0, :, 0]), -1).numpy() - sigma
        want = -np.logaddexp(lp[:, blank].sum(), lp[0, col])
        for fn in (R.mblank_autograd, R.mblank_brute):
            c, _ = fn(x, np.zeros((1, 0), np.int32), [d], [0], (col,), (d,), blank, sigma)
            assert abs(c[0] - want) < 1e-12, (fn, c, want)


def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_exports_unchanged():
    """The pruned, TDT and HAT libraries export exactly their headers, and none of the four others anything of this one."""
    I.need_lib(LIB)
    for lib, header in (("libwarprnnt_tdt.so", "rnnt_tdt.h"), ("libwarprnnt_pruned.so", "rnnt_pruned.h"),
                        ("libwarprnnt_hat.so", "rnnt_hat.h")):
        got = I.exports(os.path.join(I.LIBDIR, lib))
        assert got == I.declared(header) and not any("mblank" in s for s in got), lib
    main = I.exports(os.path.join(I.LIBDIR, "libwarprnnt.so"))
    assert "compute_rnnt_loss" in main and not any("mblank" in s for s in main)
    from warprnnt_pytorch import _lib
    assert {s for s in main if not s.startswith("_")} >= set(_lib.EXPORTS)


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for d in (4, 16, 64):
        for tag in ("F32", "F64", "BF16", "F16"):
            assert "rnnt::mblank_stats_kernel<rnnt::%s, %d>" % (tag, d) in ks
    assert {len(c["durations"]) for c in F.CASES.values()} >= {0, 1, 3, 8}


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


def test_python_refuses_bad_big_blanks():
    from warprnnt_pytorch import mblank
    for durs in ((1,), (65,), (2, 2), (4, 2), (0, 2), tuple(range(2, 11))):
        with pytest.raises(ValueError):
            mblank.MultiBlankLoss(durs, blank=20)
    for cols in ((20, 3), (3, 3), (-1, 3), (3,), (1, 2, 3)):          # the blank, a duplicate, negative, wrong counts
        with pytest.raises(ValueError):
            mblank.MultiBlankLoss((2, 4), blank=20, big_blank_columns=cols)
    with pytest.raises(ValueError):
        mblank.MultiBlankLoss((2, 4, 8), blank=2)                    # NeMo's layout needs blank >= K
    m = mblank.MultiBlankLoss((2, 4, 8), blank=3)
    assert m.columns == (2, 1, 0) and m.durations == (2, 4, 8)
    assert mblank.MultiBlankLoss((), blank=0).columns == ()
    assert mblank.MultiBlankLoss((2, 64), blank=0, big_blank_columns=(5, 1)).columns == (5, 1)
