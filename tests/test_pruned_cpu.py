"""No GPU: the pruned loss's references (tests/pruned_ref.py) against the existing ones, the prune-ranges rule's invariants, and
libwarprnnt_pruned.so's C-ABI and code objects against include/rnnt_pruned.h and tests/pruned_forms.py."""
import os
import shutil
import sys

import numpy as np
import pytest

from tests import inventory as I
from tests import pruned_forms as P
from tests import pruned_ref as R
from tests.autograd_ref import rnnt_autograd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_pruned.so", "rnnt_pruned.h"


def _problem(rng, N, T, U, A):
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    return rng.standard_normal((N, T, U, A)), labels, tl, ll


def test_full_windows_equal_the_full_loss(oracle):
    """S = L_b + 1 (= maxU for the longest sample) and starts 0: the pruned reference is autograd_ref's and the oracle's loss."""
    rng = np.random.default_rng(1)
    N, T, U, A = 4, 6, 5, 7
    x, labels, tl, ll = _problem(rng, N, T, U, A)
    ranges = np.zeros((N, T), np.int32)
    c, g = R.pruned_autograd(x, labels, ranges, tl, ll)
    c1, g1 = rnnt_autograd(x, labels, tl, ll)
    c2, g2 = oracle.rnnt_logits(x, labels, tl, ll)
    assert np.allclose(c, c1, rtol=1e-12) and np.allclose(g, g1, atol=1e-12)
    assert np.allclose(c, c2, rtol=1e-9) and np.allclose(g, g2, atol=1e-9)


def test_windows_that_miss_the_path_cost_infinity():
    rng = np.random.default_rng(2)
    T, L, S, A = 4, 5, 2, 6
    x = rng.standard_normal((1, T, S, A))
    labels = rng.integers(1, A, size=(1, L)).astype(np.int32)
    ranges = np.zeros((1, T), np.int32)                      # 4 frames, 1 step each at most: cannot reach L = 5
    assert not R.has_path(ranges[0], T, L, S)
    c, _ = R.pruned_autograd(x, labels, ranges, [T], [L])
    assert np.isposinf(c[0])


def test_narrow_windows_lose_paths():
    """Fewer paths: the pruned cost of the same logits is at least the full loss's."""
    rng = np.random.default_rng(3)
    N, T, U, A, S = 3, 8, 6, 5, 3
    x, labels, tl, ll = _problem(rng, N, T, U, A)
    tl[:] = T
    ranges = np.zeros((N, T), np.int32)
    for b in range(N):
        ranges[b] = R.ranges_rule(rng.random((T, ll[b] + 1)), T, int(ll[b]), S)
    idx = np.minimum(ranges[:, :, None] + np.arange(S), U - 1)
    xp = np.take_along_axis(x, idx[..., None].repeat(A, -1), 2)
    c, _ = R.pruned_autograd(xp, labels, ranges, tl, ll)
    c_full, _ = rnnt_autograd(x, labels, tl, ll)
    assert (c >= c_full - 1e-9).all()


@pytest.mark.parametrize("seed", range(40))
def test_ranges_rule_invariants(seed):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 30))
    S = int(rng.integers(2, 9))
    L = int(rng.integers(0, T * (S - 1) + 1))
    gam = rng.random((T, L + 1)) ** 4                         # peaky occupancies
    s = R.ranges_rule(gam, T, L, S)
    assert R.check_invariants(s, T, L, S) == [], (T, L, S, s)


@pytest.mark.parametrize("seed", range(10))
def test_ranges_rule_infeasible_branch(seed):
    rng = np.random.default_rng(100 + seed)
    T = int(rng.integers(1, 10))
    S = int(rng.integers(2, 5))
    L = T * (S - 1) + int(rng.integers(1, 5))
    s = R.ranges_rule(rng.random((T, L + 1)), T, L, S)
    assert list(s) == [min(t * (S - 1), L + 1 - S) for t in range(T)]
    assert not any(R.has_path(s, T, L, S) for _ in [0])


def test_has_path_brute_force():
    assert R.has_path([0, 0, 1], 3, 2, 2)
    assert not R.has_path([0, 0, 0], 3, 2, 2)
    assert R.has_path([0], 1, 0, 1)
    assert not R.has_path([0, 2], 2, 2, 2)                    # a gap between consecutive windows


def test_exports_equal_the_header():
    declared, exported = I.declared(HEADER), I.exports(I.need_lib(LIB))
    assert declared and exported == declared, (sorted(exported), sorted(declared))


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), P.expected_inventory())


@pytest.fixture(scope="module")
def pruned_asm():
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lattice_lin_isa as guard
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(ROOT, "warp-transducer_amd", "csrc", n) for n in P.OBJECTS.values()]
    with ThreadPoolExecutor(3) as pool:
        asms = list(pool.map(lambda s: guard.device_asm(None, s), srcs))
    return dict(zip(P.OBJECTS.values(), asms))


def test_device_code_resources_and_lattice_guards(pruned_asm, tmp_path):
    """No scratch, no spilled VGPRs (tools/check_kernel_resources.py); this library's copies of lattice_lin_kernel and
    lattice_kernel pass the two lattice ISA guards (tools/check_lattice_lin_isa.py, tools/check_lattice_asm_hazards.py)."""
    import check_kernel_resources as res
    import check_lattice_asm_hazards as hz
    import check_lattice_lin_isa as guard
    hand = seen_all = 0
    for unit, asm in pruned_asm.items():
        assert res.kernels(asm) and res.check(asm) == [], unit
        if unit != P.OBJECTS["f64"]:
            assert guard.check(asm) == [], unit
        seen, total, probs = hz.check(asm)
        assert probs == [], (unit, probs)
        hand, seen_all = hand + total, seen_all + seen
    assert seen_all and hand > 0                              # (the lattice kernels' hand-issued row accesses were looked at)
