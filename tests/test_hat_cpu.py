"""No GPU: the HAT loss's fp64 reference (tests/hat_ref.py) against brute-force path enumeration, the existing fp64 oracle fed
with hat_log_probs, a closed form and the gradient formula of include/rnnt_hat.h; and libwarprnnt_hat.so's C-ABI and code
objects against include/rnnt_hat.h and tests/hat_forms.py."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import hat_forms as F
from tests import inventory as I
from tests import hat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_hat.so", "rnnt_hat.h"


def _tiny(seed, N=3):
    rng = np.random.default_rng(2000 + seed)
    T, U, A = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(2, 7))
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    ll[1] = 0                                                     # L_b = 0
    blank = (0, A - 1, A // 2)[seed % 3]                          # first / last / interior
    x = rng.standard_normal((N, T, U, A)) * 1.5
    lab = rng.integers(0, A - 1, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    labels = lab + (lab >= blank)
    return x, labels, tl, ll, blank, rng


@pytest.mark.parametrize("seed", range(50))
def test_reference_equals_brute_force(seed):
    x, labels, tl, ll, blank, rng = _tiny(seed)
    w = rng.random(len(tl)) + 0.5
    c1, g1 = R.hat_autograd(x, labels, tl, ll, blank, w)
    c2, g2 = R.hat_brute(x, labels, tl, ll, blank, w)
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-10)
    assert not g1[~R.in_lattice_mask(x.shape, tl, ll)].any()
    assert g1[R.in_lattice_mask(x.shape, tl, ll)].any()


@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_the_oracle_fed_with_hat_log_probs(seed, oracle):
    """An independent route: the existing fp64 oracle (log-probs in, sparse gradient out) on hat_log_probs(z), its gradient
    chained through the transform by torch autograd."""
    from warprnnt_pytorch.hat import hat_log_probs
    x, labels, tl, ll, blank, _ = _tiny(seed)
    if x.shape[2] == 1:
        labels = np.zeros((x.shape[0], 0), np.int32)
    c1, g1 = R.hat_autograd(x, labels, tl, ll, blank)
    z = torch.tensor(x, requires_grad=True)
    lp = hat_log_probs(z, blank)
    assert torch.allclose(torch.log_softmax(lp, -1), lp, atol=1e-14)          # rows are normalised
    c2, g_lp = oracle.rnnt_logprobs(lp.detach().numpy(), labels, tl, ll, blank)
    mask = R.in_lattice_mask(x.shape, tl, ll)
    g_lp = np.where(mask[..., None], g_lp, 0.0)
    lp.backward(torch.tensor(g_lp))
    assert np.allclose(c1, c2, rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, z.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_closed_form_single_cell():
    """T = 1, L = 0: the one path is the terminal blank, cost = softplus(-z_blank)."""
    for zb in (-30.0, -1.0, 0.0, 2.5, 30.0):
        x = np.array([0.3, zb, -0.7]).reshape(1, 1, 1, 3)
        for fn in (R.hat_autograd, R.hat_brute):
            c, g = fn(x, np.zeros((1, 0), np.int32), [1], [0], 1)
            assert abs(c[0] - np.logaddexp(0.0, -zb)) < 1e-12
            assert abs(g[0, 0, 0, 1] - (1.0 / (1.0 + np.exp(-zb)) - 1.0)) < 1e-12 and not g[0, 0, 0, [0, 2]].any()


@pytest.mark.parametrize("seed", range(6))
def test_gradient_formula_of_the_header(seed):
    x, labels, tl, ll, blank, _ = _tiny(seed)
    _, g = R.hat_autograd(x, labels, tl, ll, blank)
    assert np.allclose(R.hat_formula(x, labels, tl, ll, blank), g, rtol=1e-12, atol=1e-14)


def test_reference_differs_from_plain_rnnt():
    x, labels, tl, ll, blank, _ = _tiny(3)
    c1, _ = R.hat_autograd(x, labels, tl, ll, blank)
    c2, _ = R.hat_autograd(x, labels, tl, ll, blank, plain=True)
    assert np.abs(c1 - c2).min() > 1e-3


def test_stable_log_sigmoid():
    """fp32: log(1 - sigmoid(80)) is -inf, logsigmoid(-80) is -80 -- why the kernels use the softplus form."""
    z = torch.tensor([80.0])
    assert torch.isinf(torch.log(1 - torch.sigmoid(z))).all()
    assert torch.nn.functional.logsigmoid(-z).item() == -80.0


def test_hat_log_probs_refuses_bad_blank():
    from warprnnt_pytorch.hat import hat_log_probs
    for blank in (-1, 4):
        with pytest.raises(ValueError):
            hat_log_probs(torch.zeros(1, 1, 1, 4), blank)


def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_exports_unchanged():
    """The pruned and TDT libraries export exactly their headers, and the main library nothing of this one."""
    I.need_lib(LIB)
    for lib, header in (("libwarprnnt_tdt.so", "rnnt_tdt.h"), ("libwarprnnt_pruned.so", "rnnt_pruned.h")):
        assert I.exports(os.path.join(I.LIBDIR, lib)) == I.declared(header), lib
    main = I.exports(os.path.join(I.LIBDIR, "libwarprnnt.so"))
    assert "compute_rnnt_loss" in main and not any("hat" in s for s in main)


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def _blank_shares_a_packet(case):
    """Some row's blank lies in a 16-byte packet that also holds elements of the neighbouring row."""
    esz = F.STORES[case["dtype"]][3]
    V, A, blank = 16 // esz, case["A"], case["blank"]
    for r in range(16):
        skip = ((case.get("off", 0) + r * A * esz) % 16) // esz
        pk = (skip + blank) // V
        if (pk == 0 and skip > 0) or (pk == (skip + A - 1) // V and (skip + A) % V != 0):
            return True
    return False


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    # hat_stats_kernel is the one user of the shared row reduction's per-element hook (csrc/rnnt_row_lse.h): for every store
    # and group size rows off a 16-byte boundary, rows that take a second round of four packets per lane, and the blank in
    # column 0, in column A - 1 and in a packet shared with the neighbouring row
    for d, (_, tag, _, esz) in F.STORES.items():
        for g in (4, 16, 64):
            cs = [c for c in F.CASES.values() if c["dtype"] == d and F.stats_group(c["A"] * esz) == g]
            assert ("rnnt::hat_stats_kernel<%s, %d>" % (tag, g)) in {k for _, k in rows} and cs
            got = [F.C.row_corners(esz, c["A"], g, c.get("off", 0)) for c in cs]
            assert any(skip for skip, _ in got) and any(rounds >= 2 for _, rounds in got), (d, g, got)
            assert any(c["blank"] == 0 for c in cs) and any(c["blank"] == c["A"] - 1 for c in cs), (d, g)
            assert any(c["blank"] == 0 and _blank_shares_a_packet(c) for c in cs), (d, g)
            assert any(c["blank"] == c["A"] - 1 and _blank_shares_a_packet(c) for c in cs), (d, g)


def test_device_code_has_no_scratch():
    """No scratch (private segment 0), no spilled VGPRs (tools/check_kernel_resources.py) in any of the three code objects."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as res
    import check_lattice_lin_isa as guard
    for unit in F.OBJECTS.values():
        asm = guard.device_asm(None, os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
        assert res.kernels(asm) and res.check(asm) == [], unit
