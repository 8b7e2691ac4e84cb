"""No GPU: the checker the side libraries' GPU tests share (tests/side_check.py) refuses each planted fault, one at a time, and
accepts the reference against itself; the stage comparison refuses an extra, a missing and an unpredicted kernel."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hat_ref as R
from tests.side_check import assert_stages, check, in_lattice_mask, stages_seen

N, T, U, A, BLANK = 3, 4, 3, 5, 2
TL, LL = np.array([4, 1, 3], np.int32), np.array([2, 0, 1], np.int32)
LABELS = np.array([[0, 3], [4, 1], [1, 0]], np.int32)
MASK = in_lattice_mask((N, T, U), TL, LL)
REF_C, REF_G = R.hat_autograd(np.random.default_rng(0).standard_normal((N, T, U, A)) * 2.0, LABELS, TL, LL, BLANK)


def _mag(ref, b):
    """|ref|, and for the blank and label columns the row's |ref| sum (tests/test_gpu_hat.py)."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    mag[..., BLANK] = np.maximum(mag[..., BLANK], rs)
    for u in range(int(LL[b])):
        mag[0, :, u, LABELS[b, u]] = np.maximum(mag[0, :, u, LABELS[b, u]], rs[0, :, u])
    return mag


def _check(got_c, got_g, ref_c=REF_C, dtype="f32", **kw):
    check(dtype, got_c, got_g, ref_c, REF_G, MASK, _mag, what="planted", **kw)


def _no_path(b=1):
    """The reference and a faithful answer with sample b made one without a path: +inf cost, NaN in-lattice gradients."""
    ref_c, got_c, got_g = REF_C.copy(), REF_C.copy(), REF_G.copy()
    ref_c[b] = got_c[b] = np.inf
    got_g[b][MASK[b]] = np.nan
    return ref_c, got_c, got_g


def test_the_reference_passes_against_itself():
    assert np.isfinite(REF_C).all() and REF_G[MASK].any() and not REF_G[~MASK].any()
    for dtype in ("f32", "f64", "bf16", "f16"):
        _check(REF_C.copy(), REF_G.copy(), dtype=dtype)
    _check(REF_C.copy(), REF_G.copy(), infinite_ok=False)
    _check(REF_C.copy(), None)
    w = np.array([0.5, 2.0, -1.5])
    _check(REF_C.copy(), REF_G * w[:, None, None, None], scale=w)
    ref_c, got_c, got_g = _no_path()
    _check(got_c, got_g, ref_c)


def test_every_gradient_ten_per_cent_short_is_refused():
    g = np.where(MASK[..., None], REF_G * 0.9, REF_G)
    with pytest.raises(AssertionError):
        _check(REF_C.copy(), g)


def test_one_tiny_padding_element_is_refused():
    g = REF_G.copy()
    g[tuple(np.argwhere(~MASK)[0])][1] = 1e-30
    with pytest.raises(AssertionError, match="padding"):
        _check(REF_C.copy(), g)


def test_one_cost_off_by_a_thousandth_is_refused():
    c = REF_C.copy()
    c[2] *= 1.0 + 1e-3
    with pytest.raises(AssertionError):
        _check(c, REF_G.copy())
    with pytest.raises(AssertionError):
        _check(c, None, infinite_ok=False)


def test_infinite_costs_must_match_position_for_position():
    ref_c, got_c, got_g = _no_path()
    with pytest.raises(AssertionError):              # +inf expected, a finite cost answered
        _check(REF_C.copy(), got_g, ref_c)
    with pytest.raises(AssertionError):              # a finite cost expected, +inf answered
        _check(got_c, got_g)
    with pytest.raises(AssertionError):              # a library without such samples: +inf in the reference is a fault
        _check(got_c, got_g, ref_c, infinite_ok=False)


def test_a_sample_without_a_path_must_hold_nan():
    ref_c, got_c, got_g = _no_path()
    got_g[1][MASK[1]] = 0.0
    with pytest.raises(AssertionError, match="no path"):
        _check(got_c, got_g, ref_c)


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_one_label_element_past_its_bound_is_refused(dtype):
    b, t, u = 0, 2, 1
    k = int(LABELS[b, u])
    assert MASK[b, t, u] and u < LL[b]
    name = {"f32": "float32", "f64": "float64", "bf16": "bfloat16", "f16": "float16"}[dtype]
    bound = O.grad_bound(REF_G[b, t, u, k], _mag(REF_G[b:b + 1], b)[0, t, u, k], name)
    g = REF_G.copy()
    g[b, t, u, k] += 0.5 * bound
    _check(REF_C.copy(), g, dtype=dtype)
    g[b, t, u, k] = REF_G[b, t, u, k] + 3.0 * bound
    with pytest.raises(AssertionError):
        _check(REF_C.copy(), g, dtype=dtype)


def test_sixteen_bit_storage_on_long_lattices_passes_a_thousandth():
    """rel = 1e-3 instead of 2^-13 past 500 diagonals: an error of 0.0045 |ref| lies between the two bf16 bounds of an
    ordinary column, (2^-8 + 2^-13) |ref| = 0.0040 |ref| and (2^-8 + 1e-3) |ref| = 0.0049 |ref|."""
    g = np.where(MASK[..., None], REF_G * 1.0045, REF_G)
    with pytest.raises(AssertionError):
        _check(REF_C.copy(), g, dtype="bf16", diagonals=500)
    _check(REF_C.copy(), g, dtype="bf16", diagonals=501)
    with pytest.raises(AssertionError):
        _check(REF_C.copy(), g, dtype="f32", diagonals=501)


def _stage_of(name):
    return {"s": "stats", "l": "lattice", "x": "other"}.get(name[0])


def test_stage_comparison():
    want = {"stats": {"s1"}, "lattice": {"l1", "l2"}}
    stages = ("stats", "lattice", "grad")
    seen = stages_seen(["s1", "memcpy", "l1", "l2", "l1"], _stage_of, stages)
    assert seen == {"stats": {"s1"}, "lattice": {"l1", "l2"}, "grad": set()}
    assert_stages("case", seen, want)
    with pytest.raises(AssertionError):              # an extra kernel in a stage
        assert_stages("case", stages_seen(["s1", "s2", "l1", "l2"], _stage_of, stages), want)
    with pytest.raises(AssertionError):              # a missing one
        assert_stages("case", stages_seen(["s1", "l1"], _stage_of, stages), want)
    with pytest.raises(AssertionError):              # a stage that is seen but neither listed nor predicted
        assert_stages("case", stages_seen(["s1", "l1", "l2", "x1"], _stage_of, stages), want)
    with pytest.raises(AssertionError):              # a predicted stage of which nothing ran
        assert_stages("case", stages_seen(["s1"], _stage_of), want)
