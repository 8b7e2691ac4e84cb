"""No GPU: the TDT loss's fp64 reference (tests/tdt_ref.py) against brute-force path enumeration and a closed form, and
libwarprnnt_tdt.so's C-ABI and code objects against include/rnnt_tdt.h and tests/tdt_forms.py."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import tdt_forms as F
from tests import tdt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_tdt.so", "rnnt_tdt.h"
SETS = [(0, 1, 2, 3, 4), (0, 2, 4), (1, 2), (1,)]


@pytest.mark.parametrize("seed", range(50))
def test_reference_equals_brute_force(seed):
    rng = np.random.default_rng(1000 + seed)
    durs = SETS[seed % len(SETS)]
    N = 3
    T, U, A = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(2, 6))
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    ll[1] = 0                                                     # L_b = 0
    blank = A - 1 if seed % 2 else 0
    sigma = 0.05 if seed % 3 == 0 else 0.0
    x = rng.standard_normal((N, T, U, A + len(durs))) * 1.5
    labels = rng.integers(0, A, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    w = rng.random(N) + 0.5
    c1, g1 = R.tdt_autograd(x, labels, tl, ll, durs, blank, sigma, w)
    c2, g2 = R.tdt_brute(x, labels, tl, ll, durs, blank, sigma, w)
    assert np.array_equal(np.isinf(c1), np.isinf(c2)), (c1, c2)
    fin = np.isfinite(c1)
    assert np.allclose(c1[fin], c2[fin], rtol=1e-12, atol=1e-12)
    assert np.allclose(g1, g2, rtol=1e-10, atol=1e-12)
    assert not g1[~R.in_lattice_mask(x.shape, tl, ll)].any()


def test_infeasible_samples_cost_infinity():
    """durations [0, 2] with an odd T_b and L_b = 0: only even frames are reachable, the final blank leaves an odd one."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 5, 1, 3 + 2))
    for fn in (R.tdt_autograd, R.tdt_brute):
        c, g = fn(x, np.zeros((2, 0), np.int32), [5, 4], [0, 0], (0, 2))
        assert np.isposinf(c[0]) and np.isfinite(c[1]) and not g[0].any()


def test_single_duration_closed_form():
    """durations = [1]: one duration column, log-softmax exactly 0.  With T_b = L_b + 1 one path survives -- the labels on the
    diagonal, then the final blank."""
    rng = np.random.default_rng(8)
    A, L = 6, 4
    T = L + 1
    x = rng.standard_normal((1, T, L + 1, A + 1))
    labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
    for blank, sigma in ((0, 0.0), (A - 1, 0.05)):
        lp = torch.log_softmax(torch.tensor(x[0, :, :, :A]), -1).numpy() - sigma
        want = -(sum(lp[u, u, labels[0, u]] for u in range(L)) + lp[L, L, blank])
        for fn in (R.tdt_autograd, R.tdt_brute):
            c, _ = fn(x, labels, [T], [L], (1,), blank, sigma)
            assert abs(c[0] - want) < 1e-12, (fn, c, want)


def test_exports_equal_the_header():
    declared, exported = I.declared(HEADER), I.exports(I.need_lib(LIB))
    assert declared and exported == declared, (sorted(exported), sorted(declared))


def test_python_refuses_bad_durations():
    from warprnnt_pytorch import tdt
    for d in ((), (1, 1), (2, 1), (-1, 1), (0,), (0, 65), tuple(range(9))):
        with pytest.raises(ValueError):
            tdt.TDTLoss(d)
    tdt.TDTLoss((0, 1, 2, 3, 4), blank=4)
    tdt.TDTLoss((1,))


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


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
