"""-m gpu: libwarprnnt_logprobs.so and warprnnt_pytorch.logprobs against the fp64 definition of tests/logprobs_ref.py.

Accuracy.  u = 2^-24 (2^-53 for fp64), m the row's maximum, all per real row:
    forward   |err(lse)|, |err(px)|, |err(py)| <= u ((C - 1) + 2 max_c |z_c - m| + |lse| + |z_y| + K_FN)
              (z_y: the gathered logit of the edge; 0 for lse)
    backward  |err(dz_c)| <= u (|gl - gx - gy| p_c (|z_c - lse| + K_FN) + 2 |dz_c|) + one rounding to the logits' type,
              p_c = exp(z_c - lse), against the reference formed from the lse the GPU returned.
K_FN = 12 covers the exp and log instructions the kernels use, counted from the instruction sequences of
csrc/rnnt_logprobs_kernels.h; every rounding is at most u relative, one ulp is 2 u.
Forward.  A term is fast_exp(x) = v_exp_f32(x * log2(e)), x = z - shift <= 0: the difference, the product and the rounded constant
perturb the exponent by up to 3 |x| u, v_exp_f32 adds its ulp, 2 u.  The sum's relative error from its terms is at most the
largest of theirs: the bound's 2 max|z - m| carries two of the three exponent roundings, and the third is at most 6 u for the
terms with |x| <= 6; a lighter term weighs less than e^-6 of the sum and its (3 |x| + 2) e^-|x| u < 0.05 u is charged to (C - 1),
of which the tree-shaped order uses only its depth.  So far 2 + 6.  When the G lanes meet, the lane's sum is rescaled by
fast_exp(m_lane - M) and multiplied: 2 + 1 (the rescaling exponent's roundings weigh as the terms' do).  logf is within one ulp
of log(sum) and shift + log one rounding of lse, which the |lse| term scales; the edge's subtraction z_y - lse is one rounding
of at most |z_y| + |lse|: 1 left over for log(sum) where |shift| outgrows |lse|.  2 + 6 + 3 + 1 = 12.
Backward.  x = z - lse is ONE rounding, the |z_c - lse| u of the bound; lp_exp is the library's expf, within one ulp (2 u) of
exp(x); lp_coef returns gl - gx - gy to one rounding of the result (1) and the product is one more (1): 4 <= 12 relative to
|coef| p_c.  A column that is the blank or the label adds its gradient in one rounding of dz, one that is both (lp_both)
sums the three terms to one rounding of dz: the 2 |dz_c| term.  fp64 uses exp() and log() of the device library, within
one to two ulp: the same count stays below 12.

Coverage.  px, py, lse and dlogits start as NaN and must be written everywhere; the logits of rows that are not real hold NaN,
as do the incoming gradients on elements that are not real: the outputs there must be -inf / exact 0 and everything else
finite.  Two calls give the same bits; dlogits == logits gives the bits of the separate call.  Every kernel form of
tests/logprobs_forms.py is run and seen to launch."""
import zlib

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import logprobs_forms as F
from tests import logprobs_ref as R
from tests.gpu_support import (CODE, COST_TOL, DEV, TORCH, assert_every_row_reached, assert_stages, check, options, place, profiled,
                               stages_seen)

pytestmark = pytest.mark.gpu

K_FN = 12.0
U_LAT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "bf16": 2.0 ** -24, "f16": 2.0 ** -24}         # the lattice type's unit roundoff
U_STORE = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}        # one rounding to the storage type
MANTISSA = {"f32": 23, "f64": 52, "bf16": 7, "f16": 10}
MIN_EXP = {"f32": -126, "f64": -1022, "bf16": -126, "f16": -14}
INF = float("inf")
WORST = {}                                              # {(dtype, "fwd" | "bwd"): the largest error / bound seen}


def _lp():
    from warprnnt_pytorch import logprobs
    return logprobs


def _np(t):
    return t.detach().double().cpu().numpy()


def _lat(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def store_rounding(ref, dtype):
    """The error one rounding of `ref` to `dtype` can have: half a quantum (the subnormal spacing below the smallest normal)."""
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** MIN_EXP[dtype])))
    return 0.5 * 2.0 ** (e - MANTISSA[dtype])


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _nan(shape, dtype, off=0):
    if 0 in tuple(shape):
        return torch.empty(tuple(shape), dtype=dtype, device=DEV)
    return place(torch.full(tuple(shape), float("nan"), dtype=dtype, device=DEV), off, dtype)


class Problem:
    """One shape on the device: logits with NaN in every row that is not real, the index tensors, the reference's arguments."""

    def __init__(self, name, dtype, K, mod, B, T, U, C, off=0, boundary="ragged", ranges=None, symbols=None, blank=None, z=None,
                 scale=3.0):
        rng = self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        case = dict(B=B, T=T, U=U, K=K)
        self.name, self.dtype, self.K, self.mod, self.off = name, dtype, K, mod, off
        self.B, self.T, self.U, self.C, self.Kp = B, T, U, C, (K if K else U)
        self.blank = int(rng.integers(0, C)) if blank is None else blank
        self.bd = F.boundary(case, rng) if isinstance(boundary, str) else boundary
        self.rg = (F.ranges(case, rng) if ranges is None else np.asarray(ranges, np.int32)) if K else None
        self.sym = rng.integers(0, C, size=(B, U - 1)).astype(np.int32) if symbols is None else np.asarray(symbols, np.int32)
        if symbols is None and U > 1:
            self.sym[0, 0] = self.blank                                             # a symbol equal to the blank
        self.real = R.real_mask(B, T, U, K, self.rg, self.bd)
        zt = torch.tensor(rng.standard_normal((B, T, self.Kp, C)) * scale if z is None else z, dtype=torch.float32).to(TORCH[dtype])
        self.z64 = zt.double().numpy()                                              # the stored values, exactly
        zt = zt.clone()
        zt[torch.tensor(~self.real)] = float("nan")
        self.z = place(zt.to(DEV), off, TORCH[dtype])
        self.d_sym = torch.tensor(self.sym, device=DEV) if U > 1 else None
        self.d_rg = torch.tensor(self.rg, device=DEV) if K else None
        self.d_bd = torch.tensor(self.bd, device=DEV) if self.bd is not None else None
        self.ref_kw = dict(K=K, ranges=self.rg, boundary=self.bd, modified=bool(mod))
        self.ref = R.forward(self.z64, self.sym, self.blank, **self.ref_kw)

    def _p(self, t):
        return None if t is None or t.numel() == 0 else t.data_ptr()

    def fwd(self):
        lat = _lat(self.dtype)
        px = _nan((self.B, self.U - 1, self.T + 1 - self.mod), lat)
        py, lse = _nan((self.B, self.U, self.T), lat), _nan((self.B, self.T, self.Kp), lat)
        st = _lp().lib().compute_rnnt_logprobs_fwd(self.z.data_ptr(), self._p(self.d_sym), self._p(self.d_rg), self.K, self._p(self.d_bd),
                                                   self.mod, self.T, self.U, self.C, self.B, self._p(px), py.data_ptr(),
                                                   lse.data_ptr(), options(self.T, self.U, self.blank), CODE[self.dtype])
        torch.cuda.synchronize()
        assert st == 0
        return px, py, lse

    def bwd(self, lse, gx, gy, gl, alias=False):
        dz = place(self.z.clone(), self.off, self.z.dtype) if alias else _nan(self.z.shape, self.z.dtype, self.off)
        src = dz if alias else self.z
        st = _lp().lib().compute_rnnt_logprobs_bwd(src.data_ptr(), lse.data_ptr(), self._p(self.d_sym), self._p(self.d_rg), self.K,
                                                   self._p(self.d_bd), self.mod, self._p(gx), gy.data_ptr(), self._p(gl), self.T,
                                                   self.U, self.C, self.B, dz.data_ptr(), options(self.T, self.U, self.blank),
                                                   CODE[self.dtype])
        torch.cuda.synchronize()
        assert st == 0
        return dz

    def grads(self, with_lse=True):
        """Incoming gradients in the lattice type, NaN on every element that is not real."""
        lat = _lat(self.dtype)
        px, py, _ = self.ref
        mk = lambda ref, live: torch.tensor(np.where(live, self.rng.standard_normal(ref.shape), np.nan), dtype=lat, device=DEV)  # noqa: E731
        return mk(px, px != -INF), mk(py, py != -INF), (mk(self.ref[2], self.real) if with_lse else None)


def check_forward(p, px, py, lse, what=""):
    """Coverage and accuracy of the three outputs; -> the largest error / bound."""
    rx, ry, rl = p.ref
    u = U_LAT[p.dtype]
    worst = 0.0
    gx, gy, gl = _np(px), _np(py), _np(lse)
    assert not np.isnan(gl).any() and not gl[~p.real].any(), (what, "lse: not written, or not exact 0 on a row that is not real")
    for name, got, ref in (("px", gx, rx), ("py", gy, ry)):
        assert got.shape == ref.shape and not np.isnan(got).any(), (what, name, "an element was not written")
        assert np.array_equal(got == -INF, ref == -INF), (what, name, "-inf exactly where no real row covers the edge")
        assert np.isfinite(got[ref != -INF]).all(), (what, name)
    sb, _ = R.lengths(p.B, p.T, p.U - 1, p.bd)
    for b, t, k, uu in R.rows(p.B, p.T, p.U, p.K, p.rg, p.bd):
        z = p.z64[b, t, k]
        base = (p.C - 1) + 2 * np.abs(z - z.max()).max() + abs(rl[b, t, k]) + K_FN
        terms = [("lse", gl[b, t, k], rl[b, t, k], 0.0), ("py", gy[b, uu, t], ry[b, uu, t], abs(z[p.blank]))]
        if uu < sb[b]:
            terms.append(("px", gx[b, uu, t], rx[b, uu, t], abs(z[min(max(int(p.sym[b, uu]), 0), p.C - 1)])))
        for name, got, ref, zy in terms:
            if ref == -INF:                                 # (a symbol outside the classes: -inf on both sides, checked above)
                continue
            ratio = abs(got - ref) / (u * (base + zy))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, name, (b, t, k), got, ref, ratio)
    return worst


def check_backward(p, lse, gx, gy, gl, dz, what=""):
    """dlogits against the reference formed from the lse the GPU returned; -> the largest error / bound."""
    l64 = _np(lse)
    ref, coef, _, _ = R.backward(p.z64, l64, p.sym, p.blank, None if gx is None else _np(gx), _np(gy), None if gl is None else _np(gl),
                                 **p.ref_kw)
    got = _np(dz)
    assert np.isfinite(got).all(), (what, "dlogits: not written everywhere, or a row or gradient that is not real was read")
    assert not got[~p.real].any(), (what, "a row that is not real is not exact zeros")
    if not p.real.any():
        return 0.0
    zl = np.where(p.real[..., None], p.z64 - l64[..., None], 0.0)
    bound = U_LAT[p.dtype] * (np.abs(coef)[..., None] * np.exp(zl) * (np.abs(zl) + K_FN) + 2 * np.abs(ref)) + store_rounding(ref, p.dtype)
    err = np.abs(got - ref)[p.real]
    ratio = err / bound[p.real]
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (what, at, err[at], bound[p.real][at])
    return float(ratio.max())


def _note(dtype, stage, ratio):
    WORST[dtype, stage] = max(WORST.get((dtype, stage), 0.0), ratio)
    print("logprobs %s %s: error / bound = %.4f (worst so far %.4f)" % (dtype, stage, ratio, WORST[dtype, stage]))


def run_and_check(p, what="", with_lse=True):
    """Forward twice, backward twice and once in place, with every check."""
    px, py, lse = p.fwd()
    _note(p.dtype, "fwd", check_forward(p, px, py, lse, what))
    again = p.fwd()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((px, py, lse), again)), (what, "two forward calls differ")
    gx, gy, gl = p.grads(with_lse)
    dz = p.bwd(lse, gx, gy, gl)
    _note(p.dtype, "bwd", check_backward(p, lse, gx, gy, gl, dz, what))
    assert torch.equal(_bits(dz), _bits(p.bwd(lse, gx, gy, gl))), (what, "two backward calls differ")
    assert torch.equal(_bits(dz), _bits(p.bwd(lse, gx, gy, gl, alias=True))), (what, "dlogits == logits differs from the separate call")
    return px, py, lse, dz


# ----------------------------------------------------------------------------- every form of tests/logprobs_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_logprobs_form(name):
    case = F.CASES[name]
    p = Problem(name, case["dtype"], case["K"], case["mod"], case["B"], case["T"], case["U"], case["C"], case.get("off", 0))
    gx, gy, gl = p.grads()

    def both():
        px, py, lse = p.fwd()
        return lse, p.bwd(lse, gx, gy, gl)

    _, names = profiled(both)
    if not any(F.stage_of(n) for n in names):           # (a profiler session now and then records no device event at all)
        _, names = profiled(both)
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, G.cus()))
    run_and_check(p, name)


def test_every_logprobs_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- the grid of the issue
@pytest.mark.parametrize("form", ["joint", "pruned"])
@pytest.mark.parametrize("mod", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_small_class_counts(dtype, mod, form):
    """C = 1 (every edge log 1 = 0), 2, 3, and the 63 / 64 / 65 around a wavefront: rows off and on the packet grid."""
    for C in (1, 2, 3, 63, 64, 65):
        what = "%s %s mod %d C %d" % (dtype, form, mod, C)
        p = Problem(what, dtype, 2 if form == "pruned" else 0, mod, 3, 4, 4, C)
        px, py, lse, _ = run_and_check(p, what)
        if C == 1:
            assert not py[py != -INF].any() and not px[px != -INF].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ["U1", "K1", "KU", "T1"])
def test_degenerate_extents(dtype, shape):
    """U = 1 (px is empty), K = 1, K = U (every start is 0), T = 1; both types."""
    K, B, T, U = {"U1": (0, 2, 3, 1), "K1": (1, 3, 4, 3), "KU": (3, 3, 4, 3), "T1": (0, 3, 1, 3)}[shape]
    for mod in (0, 1):
        what = "%s %s mod %d" % (dtype, shape, mod)
        p = Problem(what, dtype, K, mod, B, T, U, 5, boundary=None if shape == "T1" else "ragged")
        px, *_ = run_and_check(p, what)
        assert px.shape == (B, U - 1, T + 1 - mod)
    if shape == "U1":                                    # and the pruned form of it: K = U = 1
        run_and_check(Problem(dtype + " U1 pruned", dtype, 1, 0, 2, 3, 1, 5), "U1 pruned")


@pytest.mark.parametrize("along", ["T", "U"])
@pytest.mark.parametrize("n", [F.TILE - 1, F.TILE, F.TILE + 1])
def test_output_block_edges(along, n):
    """The outputs are written in blocks of F.TILE consecutive positions of the (b, u, t) order: T and U one short of, at and
    one past it, joint and pruned (K = 2, starts anywhere in [0, U - 2])."""
    T, U = (n, 2) if along == "T" else (2, n)
    for K, mod in ((0, 0), (2, 1)):
        what = "%s = %d K %d" % (along, n, K)
        run_and_check(Problem(what, "f32", K, mod, 2, T, U, 3), what)


def test_ranges_at_both_ends_and_not_monotone():
    rg = np.array([[0, 3, 0, 3, 1], [3, 3, 0, 0, 2]], np.int32)           # U - K = 3
    for mod in (0, 1):
        p = Problem("ends %d" % mod, "f32", 2, mod, 2, 5, 5, 6, boundary=None, ranges=rg)
        px, py, _, _ = run_and_check(p, "ends")
        assert bool((py[0, :, 1] == -INF).tolist() == [True, True, True, False, False])
    # starts outside [0, U - K] are clamped into it: the rows and the bits of the clamped starts
    q = Problem("ends 0", "f32", 2, 0, 2, 5, 5, 6, boundary=None, ranges=rg + np.array([[-7, 9, 0, 9, 0], [9, 9, -1, -1, 0]], np.int32))
    p = Problem("ends 0", "f32", 2, 0, 2, 5, 5, 6, boundary=None, ranges=rg)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(p.fwd(), q.fwd()))


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_batch_of_empty_full_and_unbounded_samples(dtype):
    """T_b = 0, S_b = 0, a full sample, a sample with both; then boundary = None; boundary values outside [0, S] x [0, T] clamp."""
    B, T, U, C = 4, 5, 4, 9
    bd = np.array([[0, 0, 3, 5], [0, 0, 2, 0], [0, 0, 0, 4], [0, 0, 0, 0]], np.int64)
    for K in (0, 2):
        run_and_check(Problem("batch %d" % K, dtype, K, 0, B, T, U, C, boundary=bd), "batch")
        run_and_check(Problem("batch none %d" % K, dtype, K, 1, B, T, U, C, boundary=None), "no boundary")
    wild = np.array([[5, -3, 9, 77], [0, 0, -2, 5], [0, 0, 3, -1], [1, 1, 3, 5]], np.int64)
    p = Problem("clamped", dtype, 0, 0, B, T, U, C, boundary=wild)
    assert p.real[0].all() and p.real[1, :, 0].all() and not p.real[1, :, 1:].any() and not p.real[2].any()
    run_and_check(p, "clamped")


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_poisoned_rows_poison_only_themselves(dtype):
    """-inf entries beside a finite one behave as torch's log_softmax (-inf edge, zero gradient there); a row of all -inf, a
    NaN row and a +inf row give NaN in their own lse, edges and gradient, and nothing else changes a bit."""
    B, T, U, C = 1, 5, 3, 20
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B, T, U, C))
    clean = Problem("poison", dtype, 0, 0, B, T, U, C, boundary=None, z=z, blank=0, symbols=[[1, 2]])
    z2 = z.copy()
    z2[0, 0, 0, 1] = z2[0, 0, 0, 7] = -INF                 # the label of (t = 0, u = 0) and a bystander
    z2[0, 1, 1] = -INF
    z2[0, 2, 0, 3] = np.nan
    z2[0, 3, 2, 4] = INF
    p = Problem("poison", dtype, 0, 0, B, T, U, C, boundary=None, z=z2, blank=0, symbols=[[1, 2]])
    bad = np.zeros((B, T, U), bool)
    bad[0, 1, 1] = bad[0, 2, 0] = bad[0, 3, 2] = True
    touched = bad.copy()
    touched[0, 0, 0] = True
    (px, py, lse), (cx, cy, cl) = p.fwd(), clean.fwd()
    gl, gpy = _np(lse), _np(py)
    assert np.isnan(gl[bad]).all() and np.isfinite(gl[~bad]).all()
    assert np.isnan(gpy.transpose(0, 2, 1)[bad]).all() and np.isfinite(gpy.transpose(0, 2, 1)[~bad]).all()
    assert px[0, 0, 0].item() == -INF and np.isnan(px[0, 1, 1].item()) and np.isnan(px[0, 0, 2].item())
    same = torch.tensor(~touched, device=DEV)
    assert torch.equal(_bits(lse[same]), _bits(cl[same])) and torch.equal(_bits(py.transpose(1, 2)[same]), _bits(cy.transpose(1, 2)[same]))
    ref = torch.log_softmax(torch.tensor(p.z64[0, 0, 0]), 0).numpy()
    assert abs(gpy[0, 0, 0] - ref[0]) <= U_LAT[dtype] * (C + 2 * 10 + abs(ref[0]) + K_FN)
    lat = _lat(dtype)
    ones = lambda t: torch.ones_like(t, dtype=lat)          # noqa: E731
    dz, dc = p.bwd(lse, ones(px), ones(py), None), clean.bwd(cl, ones(cx), ones(cy), None)
    g = _np(dz)
    assert np.isnan(g[bad]).all() and np.isfinite(g[~bad]).all()
    assert torch.equal(_bits(dz[same]), _bits(dc[same]))
    # the -inf label: the edge's own gradient arrives whole, the bystander gets exactly 0
    assert g[0, 0, 0, 1] == 1.0 and g[0, 0, 0, 7] == 0.0


def test_a_symbol_outside_the_classes_is_minus_inf_without_gradient():
    p = Problem("outside", "f32", 0, 0, 2, 3, 3, 6, boundary=None, symbols=[[6, 2], [-1, 100000]])
    px, py, lse, dz = run_and_check(p, "outside")
    assert (px[0, 0] == -INF).all() and (px[1] == -INF).all() and torch.isfinite(px[0, 1, :3]).all()


# ----------------------------------------------------------------------------- the Python module
def _ragged(B, T, U, C, blank, rng, dtype=torch.float64):
    tl = np.array([T, T - 2, T - 1, T - 3][:B], np.int32)
    ll = np.array([U - 1, 1, 0, 2][:B], np.int32)
    labels = rng.choice([c for c in range(C) if c != blank], size=(B, U - 1)).astype(np.int32)
    bd = np.stack([np.zeros(B, np.int64), np.zeros(B, np.int64), ll.astype(np.int64), tl.astype(np.int64)], 1)
    return tl, ll, labels, bd


def _mag(ref, labels, u_of, ll, blank):
    """The size of the terms of every gradient element, the losses' own rule: |ref|, and for the blank and label columns the
    row's |ref| sum (they carry the subtracted posteriors).  u_of (B, T, K'): the lattice row of each row."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    mag[..., blank] = np.maximum(mag[..., blank], rs)
    for b, t, k in zip(*np.nonzero((u_of >= 0) & (u_of < np.asarray(ll)[:, None, None]))):
        lab = int(labels[b, u_of[b, t, k]])
        mag[b, t, k, lab] = max(mag[b, t, k, lab], rs[b, t, k])
    return mag


@pytest.mark.parametrize("form,mod", [("joint", 0), ("joint", 1), ("pruned", 0), ("pruned", 1)])
def test_end_to_end_through_mi_equals_the_loss(form, mod):
    """get_rnnt_logprobs_* -> mutual_information_recursion on one small ragged batch, fp64: -scores is the cost of RNNTLoss
    (joint regular), MonotonicRNNTLoss (joint modified) or PrunedStreamingRNNTLoss at delay_penalty = 0 (pruned), and the logits
    gradient chained through both libraries is that loss's."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.mi import mutual_information_recursion
    from warprnnt_pytorch.mono import MonotonicRNNTLoss
    from warprnnt_pytorch.pstream import PrunedStreamingRNNTLoss
    B, T, U, C, blank, K = 4, 9, 5, 11, 3, 3
    rng = np.random.default_rng(23 + mod)
    tl, ll, labels, bd = _ragged(B, T, U, C, blank, rng)
    lab, ttl, tll, tbd = G.dev(labels, tl, ll, bd)
    rtype = "modified" if mod else "regular"
    if form == "joint":
        x = torch.tensor(rng.standard_normal((B, T, U, C)) * 2, dtype=torch.float64, device=DEV)
        loss_fn = (MonotonicRNNTLoss if mod else RNNTLoss)(blank=blank, reduction="none")
        u_of = np.broadcast_to(np.arange(U)[None, None, :], (B, T, U))
        args, edges = (), lambda z: _lp().get_rnnt_logprobs_joint(z, lab, blank, tbd, rtype)      # noqa: E731
    else:
        starts = np.zeros((B, T), np.int32)
        for b in range(B):                                  # monotone windows that hold a path: steps of at most K - 1
            top = max(int(ll[b]) - K + 1, 0)
            starts[b, :tl[b]] = np.round(np.arange(tl[b]) * top / max(tl[b] - 1, 1)).astype(np.int32)
        rg, = G.dev(starts)
        x = torch.tensor(rng.standard_normal((B, T, K, C)) * 2, dtype=torch.float64, device=DEV)
        loss_fn = PrunedStreamingRNNTLoss(blank=blank, rnnt_type=rtype, delay_penalty=0.0, reduction="none")
        u_of = starts[:, :, None] + np.arange(K)[None, None, :]
        args, edges = (rg,), lambda z: _lp().get_rnnt_logprobs_pruned(z, lab, rg, blank, tbd, rtype)      # noqa: E731
    xa = x.clone().requires_grad_()
    cost = loss_fn(xa, lab, ttl, tll, *args)
    cost.sum().backward()
    assert torch.isfinite(cost).all()
    xb = x.clone().requires_grad_()
    px, py = edges(xb)
    scores = mutual_information_recursion(px, py, tbd)
    (-scores).sum().backward()
    mask = (np.arange(T)[None, :, None] < tl[:, None, None]) & (u_of <= ll[:, None, None])
    check("f64", _np(-scores), _np(xb.grad), _np(cost), _np(xa.grad), mask,
          lambda ref, b: _mag(ref, labels[b:b + 1], u_of[b:b + 1], ll[b:b + 1], blank), what="%s %s" % (form, rtype),
          infinite_ok=False)
    assert COST_TOL["f64"] == 1e-9


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_autograd_through_all_three_outputs(dtype):
    """The Python functions on int64 symbols and k2's (B, T, K) ranges: outputs and the gradient of
    sum(w px) + sum(w py) + sum(lse^2) -- the z-loss -- against the reference."""
    B, T, U, C, K = 3, 4, 4, 10, 2
    for form, mod in (("joint", 0), ("pruned", 1)):
        p = Problem("autograd %s %s" % (dtype, form), dtype, K if form == "pruned" else 0, mod, B, T, U, C)
        z = torch.nan_to_num(p.z.detach().clone(), nan=0.0).requires_grad_()
        sym = p.d_sym.long()
        rtype = "modified" if mod else "regular"
        k2_ranges = p.d_rg.long().unsqueeze(-1) + torch.arange(K, device=DEV) if form == "pruned" else None

        def edges():
            if form == "joint":
                return _lp().get_rnnt_logprobs_joint(z, sym, p.blank, p.d_bd, rtype, return_lse=True)
            return _lp().get_rnnt_logprobs_pruned(z, sym, k2_ranges, p.blank, p.d_bd, rtype, return_lse=True)

        px, py, lse = edges()
        q = Problem(p.name, dtype, p.K, mod, B, T, U, C)
        q.z64 = np.where(p.real[..., None], p.z64, 0.0)
        _note(dtype, "fwd", check_forward(q, px, py, lse, form))
        gx, gy, _ = p.grads(False)
        zero = torch.zeros((), dtype=px.dtype, device=DEV)
        loss = (torch.where(px == -INF, zero, px) * torch.nan_to_num(gx)).sum() \
            + (torch.where(py == -INF, zero, py) * torch.nan_to_num(gy)).sum() + (lse ** 2).sum()
        loss.backward()
        assert z.grad.dtype == z.dtype and z.grad.shape == z.shape
        _note(dtype, "bwd", check_backward(q, lse, gx, gy, 2 * lse.detach(), z.grad, form + " z-loss"))
        # lse alone, and (px, py) without lse
        z.grad = None
        edges()[2].pow(2).sum().backward()
        check_backward(q, lse, torch.zeros_like(gx), torch.zeros_like(gy), 2 * lse.detach(), z.grad, form + " lse only")


def test_python_validation_on_the_device():
    lp = _lp()
    z = torch.zeros(2, 3, 3, 5, device=DEV)
    zp = torch.zeros(2, 3, 2, 5, device=DEV)
    sym = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    rg = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    bd = torch.tensor([[0, 0, 2, 3], [0, 0, 1, 2]], device=DEV)
    assert len(lp.get_rnnt_logprobs_joint(z, sym, 0, bd)) == 2 and len(lp.get_rnnt_logprobs_pruned(zp, sym, rg, 0, bd, return_lse=True)) == 3
    with pytest.raises(ValueError, match=r"symbols must be in \[0, C\)"):
        lp.get_rnnt_logprobs_joint(z, sym + 5, 0)
    with pytest.raises(ValueError, match="ranges must start in"):
        lp.get_rnnt_logprobs_pruned(zp, sym, rg + 2, 0)
    for bad in ([[0, 0, 3, 3], [0, 0, 1, 2]], [[0, 0, 2, 4], [0, 0, 1, 2]], [[1, 0, 2, 3], [0, 0, 1, 2]], [[0, 0, 2, 3], [0, 1, 1, 2]]):
        with pytest.raises(ValueError, match="boundary rows must be"):
            lp.get_rnnt_logprobs_joint(z, sym, 0, torch.tensor(bad, device=DEV))
    px, _ = lp.get_rnnt_logprobs_joint(z, sym + 5, 0, validate=False)                 # unchecked: -inf, nothing faults
    assert (px == -INF).all()
    with pytest.raises(ValueError, match="joint logits must be"):
        lp.get_rnnt_logprobs_joint(zp, sym, 0)
    with pytest.raises(ValueError, match=r"termination_symbol must be in \[0, C\)"):
        lp.get_rnnt_logprobs_joint(z, sym, 5)
    with pytest.raises(ValueError, match="constrained|'regular' or 'modified'"):
        lp.get_rnnt_logprobs_joint(z, sym, 0, rnnt_type="constrained")


def test_hip_graph_capture_and_replay():
    """validate=False only enqueues: forward + backward captured in one graph on a single stream without branches, replayed
    once on new logits: the bits of the eager call."""
    lp = _lp()
    p = Problem("graph", "f32", 2, 0, 3, 6, 4, 16)
    lp.lib()
    sym, rg, bd = p.d_sym, p.d_rg, p.d_bd
    gx, gy, gl = (torch.nan_to_num(g) for g in p.grads())
    side = torch.cuda.Stream()                           # the leaf, warm-up and capture on ONE stream: the graph has no branch
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = torch.zeros_like(p.z).requires_grad_()

    def step():                                          # (autograd.grad: no gradient accumulator, whose stream is another)
        px, py, lse = lp.get_rnnt_logprobs_pruned(z, sym, rg, p.blank, bd, return_lse=True, validate=False)
        grad, = torch.autograd.grad([px, py, lse], [z], [gx, gy, gl])
        return px, py, lse, grad

    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        z.copy_(torch.nan_to_num(p.z))
    graph.replay()
    torch.cuda.synchronize()
    captured = [t.clone() for t in outs]
    eager = step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(captured, eager))
    assert torch.isfinite(captured[2]).all() and captured[3].abs().sum() > 0


def test_beyond_2_to_the_31_elements_bf16():
    """One bf16 case just over 2^31 elements, forward and backward: the first and last rows and the rows either side of element
    2^31 against the reference."""
    B, T, U, C = 1, (1 << 20) + 4, 2, 1024
    rows = B * T * U
    assert rows * C > 2 ** 31 and (2 ** 31) % C == 0
    z = torch.empty((B, T, U, C), dtype=torch.bfloat16, device=DEV)
    flat = z.view(-1)
    for at in range(0, flat.numel(), 1 << 28):
        flat[at:at + (1 << 28)].normal_(0, 2)
    rng = np.random.default_rng(31)
    sym = torch.tensor(rng.integers(0, C, size=(B, 1)).astype(np.int32), device=DEV)
    blank = 7
    lat = torch.float32
    px = torch.full((B, 1, T + 1), float("nan"), dtype=lat, device=DEV)
    py = torch.full((B, U, T), float("nan"), dtype=lat, device=DEV)
    lse = torch.full((B, T, U), float("nan"), dtype=lat, device=DEV)
    lib = _lp().lib()
    opt = options(T, U, blank)
    assert lib.compute_rnnt_logprobs_fwd(z.data_ptr(), sym.data_ptr(), None, 0, None, 0, T, U, C, B, px.data_ptr(), py.data_ptr(),
                                         lse.data_ptr(), opt, CODE["bf16"]) == 0
    gx, gy = torch.randn_like(px), torch.randn_like(py)
    dz = torch.full_like(z, float("nan"))
    assert lib.compute_rnnt_logprobs_bwd(z.data_ptr(), lse.data_ptr(), sym.data_ptr(), None, 0, None, 0, gx.data_ptr(), gy.data_ptr(),
                                         None, T, U, C, B, dz.data_ptr(), opt, CODE["bf16"]) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(lse).any() and not torch.isnan(py).any() and not torch.isnan(px).any()
    assert bool((px[:, :, T] == -INF).all()) and bool(torch.isfinite(px[:, :, :T]).all())
    mid = (2 ** 31) // C                                                 # the row that starts at element 2^31
    u = U_LAT["bf16"]
    s = int(sym[0, 0])
    for r in (0, 1, mid - 1, mid, rows - 2, rows - 1):
        t, k = divmod(r, U)
        zr = z[0, t, k].double().cpu().numpy()
        ref_l = R.row_lse(zr)
        base = (C - 1) + 2 * np.abs(zr - zr.max()).max() + abs(ref_l) + K_FN
        assert abs(lse[0, t, k].item() - ref_l) <= u * base, r
        assert abs(py[0, k, t].item() - (zr[blank] - ref_l)) <= u * (base + abs(zr[blank])), r
        g_x = gx[0, 0, t].item() if k == 0 else 0.0
        g_y, l = gy[0, k, t].item(), float(lse[0, t, k].item())
        if k == 0:
            assert abs(px[0, 0, t].item() - (zr[s] - ref_l)) <= u * (base + abs(zr[s])), r
        coef = -g_x - g_y
        ref = coef * np.exp(zr - l)
        ref[blank] += g_y
        if k == 0:
            ref[s] += g_x
        bound = u * (abs(coef) * np.exp(zr - l) * (np.abs(zr - l) + K_FN) + 2 * np.abs(ref)) + store_rounding(ref, "bf16")
        assert (np.abs(dz[0, t, k].double().cpu().numpy() - ref) <= bound).all(), r
    # every row was written: a strided sample of the gradient, and its last packet
    assert bool(torch.isfinite(dz.view(-1)[:: 4099]).all()) and bool(torch.isfinite(dz.view(-1)[-8:]).all())


def test_peak_memory_holds_no_tensor_sized_intermediate():
    """Forward + backward of a mid-size case: the peak stays within logits + dlogits + the small tensors (px, py, lse and their
    gradients, the index tensors) + 1 %."""
    lp = _lp()
    B, T, U, C = 8, 64, 16, 1024
    rng = np.random.default_rng(3)
    z = torch.randn((B, T, U, C), device=DEV).requires_grad_()
    sym = torch.tensor(rng.integers(0, C, size=(B, U - 1)).astype(np.int32), device=DEV)
    bd = torch.tensor(F.boundary(dict(B=B, T=T, U=U), rng), device=DEV)
    gx, gy, gl = torch.randn((B, U - 1, T + 1), device=DEV), torch.randn((B, U, T), device=DEV), torch.randn((B, T, U), device=DEV)
    lp.lib()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    px, py, lse = lp.get_rnnt_logprobs_joint(z, sym, 0, bd, return_lse=True, validate=False)
    torch.autograd.backward([px, py, lse], [gx, gy, gl])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)       # noqa: E731
    small = nbytes(px, py, lse)
    allowed = nbytes(z.grad) + small + 0.01 * (nbytes(z, z.grad) + small + nbytes(gx, gy, gl, sym, bd))
    print("logprobs peak memory: %d bytes over the inputs, %d allowed, dlogits %d" % (peak, allowed, nbytes(z.grad)))
    assert z.grad is not None and peak <= allowed, (peak, allowed)


def test_zz_worst_error_ratios_stay_below_one():
    """The ledger of this module's accuracy checks (printed for EXPERIMENTS.md section 23)."""
    for key in sorted(WORST):
        print("logprobs worst error / bound", key, "%.4f" % WORST[key])
    assert all(v <= 1.0 for v in WORST.values())
