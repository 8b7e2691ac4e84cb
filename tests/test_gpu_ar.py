"""-m gpu: the alignment-restricted RNN-T loss (include/rnnt_ar.h, libwarprnnt_ar.so).

Every case of tests/ar_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules predict
run, stage by stage.  Costs and gradients go through gpu_support.check against the fp64 autograd reference of
tests/ar_ref.py: costs at COST_TOL, gradients per element at oracle.grad_bound with mag = |ref| and, for the blank and label
columns, the row's |ref| sum.  Lengths and windows from the table's generators (a full sample, T_b = 1, L_b = 0, a fully
pinned sample, an unrestricted one), NaN in every row outside the band (never read) and gradient buffers that start as NaN
(those rows must come back as exact zeros).  A negative control compares against the plain RNN-T loss and must fail.  Then
unrestricted windows against RNNTLoss, windows from rnnt_align, the call forms, bit-identical reruns and workspaces, the
invalid arguments, the non-finite cases of the header, infeasible windows, a label on the blank column, the autograd module, a
HIP-graph capture, two long utterances and one bf16 tensor past 2^31 elements."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import ar_forms as F
from tests import ar_ref as R
from tests import gpu_support as G
from tests.gpu_support import (CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check,
                               dev, options, place, profiled, stages_seen)

pytestmark = pytest.mark.gpu


def _ar():
    from warprnnt_pytorch import ar
    return ar


def _problem(name, dtype, N, T, U, A, lengths, wins, rng=None, scale=2.0, blank=None):
    """Logits with NaN in every row outside the band (padding and in-lattice alike), labels over all of [0, A) but the
    blank, the lengths, the windows and the mask the check uses: the band, or the whole lattice of a sample without a path."""
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = np.asarray(lengths[0], np.int32), np.asarray(lengths[1], np.int32)
    lo, hi = np.asarray(wins[0], np.int32).reshape(N, U - 1), np.asarray(wins[1], np.int32).reshape(N, U - 1)
    allowed = [c for c in range(A) if c != blank] or [0]
    labels = rng.choice(allowed, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * scale, dtype=torch.float32).to(TORCH[dtype])
    band = R.band_mask((N, T, U), tl, ll, lo, hi)
    x[torch.tensor(~band)] = float("nan")
    mask = band.copy()
    inl = R.in_lattice_mask((N, T, U), tl, ll)
    for b in range(N):
        if not R.bounds(tl[b], ll[b], lo[b], hi[b])[2]:
            mask[b] = inl[b]
    return x, labels, tl, ll, lo, hi, mask


def _table_problem(name, dtype, N, T, U, A, blank, seed=None):
    rng = np.random.default_rng(zlib.crc32(name.encode()) if seed is None else seed)
    case = dict(N=N, T=T, U=U)
    tl, ll = F.lengths(case, rng)
    return _problem(name, dtype, N, T, U, A, (tl, ll), F.windows(case, tl, ll, rng), rng=rng, blank=blank)


def call(x, labels, tl, ll, lo, hi, blank=0, form="one", scale=None, grads=None, stream=None, null=(), ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host."""
    m = _ar()
    N, T, U, A = x.shape
    code = CODE[NAME[x.dtype]]
    pad = np.zeros((N, 1), np.int32)
    lab, ttl, tll, tlo, thi = dev(labels if labels.size else pad, tl, ll, lo if lo.size else pad, hi if hi.size else pad)
    opt = options(T, U, blank, stream)
    lib = m.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), None if "lo" in null else tlo.data_ptr(),
            None if "hi" in null else thi.data_ptr(), A, N)
    return call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_rnnt_loss_ar(x.data_ptr(), gp, *lens, costs, ws, opt, code),
        lambda costs, ws: lib.compute_rnnt_loss_ar_fwd(x.data_ptr(), *lens, costs, ws, opt, code, 1),
        lambda gp, sc, ws: lib.compute_rnnt_loss_ar_bwd(x.data_ptr(), gp, sc, A, N, ws, opt, code),
        m.workspace_bytes(T, U, N, code), scale, grads, stream, ws)


def _reference(x, labels, tl, ll, lo, hi, blank=0, weights=None):
    xr = torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()
    return R.ar_autograd(xr, labels, tl, ll, lo, hi, blank, weights)


def _mag(ref, labels, ll, blank):
    """The size of the terms of every gradient element: |ref|, and for the blank and label columns the row's |ref| sum
    (they carry the subtracted posteriors)."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    mag[..., blank] = np.maximum(mag[..., blank], rs)
    N, T, U, _ = ref.shape
    for b in range(N):
        for u in range(min(U, int(ll[b]))):
            lab = int(labels[b, u])
            mag[b, :, u, lab] = np.maximum(mag[b, :, u, lab], rs[b, :, u])
    return mag


def _check(dtype, got_c, got_g, ref_c, ref_g, mask, labels, ll, blank, scale=None, what=""):
    check(dtype, got_c, got_g, ref_c, ref_g, mask, lambda ref, b: _mag(ref, labels[b:b + 1], ll[b:b + 1], blank), scale, what,
          diagonals=mask.shape[1] + mask.shape[2] - 1)


# ----------------------------------------------------------------------------- every form of tests/ar_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_ar_form(name):
    case = F.CASES[name]
    cus = G.cus()
    N, T, U, A, dtype, blank = case["N"], case["T"], case["U"], case["A"], case["dtype"], case["blank"]
    x, labels, tl, ll, lo, hi, mask = _table_problem(name, dtype, N, T, U, A, blank)
    off = case.get("off", 0)
    xv = place(x.to(DEV), off, x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, lo, hi, blank, "one", grads=gv))
    if st == 0 and not names:                        # (a profiler session now and then records no device event at all:
        gv.fill_(float("nan"))                       #  one more session, judged as the first would have been)
        (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, lo, hi, blank, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, cus))
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank)
    assert np.isfinite(rc).all()                     # (the generated windows are feasible)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what=name)


def test_every_ar_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_negative_control_plain_rnnt_is_refused(dtype):
    """The same comparison against the plain RNN-T loss must fail: the check cannot pass on the unrestricted loss.  Windows
    with a slack of at most one frame, every sample with 1 <= L_b < T_b."""
    N, T, U, A, blank = 4, 9, 7, 12, 11
    tl, ll = np.array([9, 5, 7, 3], np.int32), np.array([6, 2, 1, 2], np.int32)
    rng = np.random.default_rng(zlib.crc32(("neg_" + dtype).encode()))
    lo, hi, _ = R.windows(rng, tl, ll, U, max_slack=1, wide=False)
    x, labels, tl, ll, lo, hi, mask = _problem("neg_" + dtype, dtype, N, T, U, A, (tl, ll), (lo, hi), rng=rng, blank=blank)
    st, c, g = call(x.to(DEV), labels, tl, ll, lo, hi, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what="restricted")
    pc, pg = O.rnnt_logits(torch.nan_to_num(x.double(), nan=0.0).numpy(), labels, tl, ll, blank)
    assert (np.abs(pc - rc) >= 100 * COST_TOL[dtype]).all(), (pc, rc)
    with pytest.raises(AssertionError):
        _check(dtype, c, None, pc, pg, mask, labels, ll, blank, what="plain costs")
    with pytest.raises(AssertionError):
        _check(dtype, rc, g, rc, pg, R.in_lattice_mask(mask.shape, tl, ll), labels, ll, blank, what="plain gradients")
    with pytest.raises(AssertionError):
        _check(dtype, rc, g, rc, pg, mask, labels, ll, blank, what="plain gradients inside the band")


def test_unrestricted_windows_are_rnntloss():
    """lo <= 0, hi >= T_b - 1 for every label: against RNNTLoss on the same tensor, fp64, on the GPU."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.ar import rnnt_loss_ar
    N, T, U, A, blank = 4, 12, 5, 37, 9
    rng = np.random.default_rng(17)
    tl, ll = np.array([12, 1, 7, 9], np.int32), np.array([4, 2, 0, 3], np.int32)
    labels = rng.choice([c for c in range(A) if c != blank], size=(N, U - 1)).astype(np.int32)
    lo, hi = np.full((N, U - 1), -3, np.int32), np.full((N, U - 1), 1 << 20, np.int32)
    lo[0], hi[0] = 0, tl[0] - 1                                  # the tightest unrestricted window
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * 2, dtype=torch.float64, device=DEV)
    lab, ttl, tll, tlo, thi = dev(labels, tl, ll, lo, hi)
    xa = x.clone().requires_grad_()
    la = rnnt_loss_ar(xa, lab, ttl, tll, tlo, thi, blank, "none", validate=False)
    la.sum().backward()
    xb = x.clone().requires_grad_()
    lb = RNNTLoss(blank=blank, reduction="none", validate=False)(xb, lab, ttl, tll)
    lb.sum().backward()
    assert torch.allclose(la, lb, rtol=1e-9, atol=0), (la, lb)
    mask = R.band_mask((N, T, U), tl, ll, lo, hi)
    assert np.array_equal(mask, R.in_lattice_mask((N, T, U), tl, ll))
    ga, gb = xa.grad.cpu().numpy(), xb.grad.cpu().numpy()
    assert not ga[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, ll, blank)[mask], torch.float64, what="cross-check")


def test_windows_from_rnnt_align():
    """Windows of no slack around the best path leave that path alone: cost = -score of rnnt_align.  Two frames of slack on
    either side lower the cost, unrestricted windows lower it further (or leave it)."""
    from warprnnt_pytorch import rnnt_align
    from warprnnt_pytorch.ar import alignment_windows, rnnt_loss_ar
    N, T, U, A, blank = 4, 14, 6, 11, 0
    rng = np.random.default_rng(23)
    tl, ll = np.array([14, 9, 14, 5], np.int32), np.array([5, 3, 0, 5], np.int32)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * 2, dtype=torch.float64, device=DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    score, frames = rnnt_align(x, lab, ttl, tll, blank)
    assert frames.dtype == torch.int32 and torch.isfinite(score).all()
    costs = []
    for left, right in ((0, 0), (2, 2), (T, T)):
        lo, hi = alignment_windows(frames, left, right)
        assert lo.dtype == torch.int32 and lo.device == frames.device
        costs.append(rnnt_loss_ar(x, lab, ttl, tll, lo, hi, blank, "none"))
    assert torch.allclose(costs[0], -score, rtol=1e-9, atol=0), (costs[0], score)
    some = torch.tensor(ll > 0)
    assert (costs[1][some] < costs[0][some]).all() and (costs[2] <= costs[1]).all()
    assert torch.equal(costs[0][~some], costs[2][~some])


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("dtype,U", [("f32", 9), ("bf16", 9), ("f32", 66)])
def test_call_forms_agree(dtype, U):
    N, T, A, blank = 5, 11, 130, 129
    x, labels, tl, ll, lo, hi, mask = _table_problem("forms_" + dtype, dtype, N, T, U, A, blank, seed=U)
    xd = x.to(DEV)
    st, c1, g1 = call(xd, labels, tl, ll, lo, hi, blank, "one")
    assert st == 0
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    st, c2, g2 = call(xd, labels, tl, ll, lo, hi, blank, "two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank, weights=scale)
    _check(dtype, c2, g2, rc, rg, mask, labels, ll, blank, what="two-phase")
    st, c2b, g2b = call(xd, labels, tl, ll, lo, hi, blank, "two", scale=np.ones(N))
    assert st == 0 and np.array_equal(c1, c2b) and np.array_equal(g2b, g1)            # bit for bit at scale 1
    xi = xd.clone()
    st, c3, g3 = call(xi, labels, tl, ll, lo, hi, blank, "inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1)
    st, c4, _ = call(xd, labels, tl, ll, lo, hi, blank, "score")
    assert st == 0 and np.array_equal(c1, c4)
    st, c5, g5 = call(xd, labels, tl, ll, lo, hi, blank, "host", grads=torch.full_like(xd, float("nan")))
    assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5) and np.array_equal(g5, g1)
    # a second run: identical bits
    st, c6, g6 = call(xd, labels, tl, ll, lo, hi, blank, "one")
    assert st == 0 and np.array_equal(c1, c6) and np.array_equal(g1, g6)


@pytest.mark.parametrize("U", [6, 70])
def test_workspace_contents_do_not_matter(U):
    """A workspace full of 0xFF bytes (NaN as values, -1 as flags and bounds) gives the bits a zeroed one gives: nothing an
    earlier call left reaches arithmetic."""
    m = _ar()
    N, T, A, blank = 5, 13, 19, 3
    x, labels, tl, ll, lo, hi, mask = _table_problem("ws", "f32", N, T, U, A, blank, seed=U)
    xd = x.to(DEV)
    lab, ttl, tll, tlo, thi = dev(labels, tl, ll, lo, hi)
    out = []
    for fill in (0, 255):
        ws = torch.full((m.workspace_bytes(T, U, N, 0),), fill, dtype=torch.uint8, device=DEV)
        costs = torch.full((N,), float("nan"), device=DEV)
        g = torch.full_like(xd, float("nan"))
        st = m.lib().compute_rnnt_loss_ar(xd.data_ptr(), g.data_ptr(), lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(),
                                          tlo.data_ptr(), thi.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(),
                                          options(T, U, blank), 0)
        torch.cuda.synchronize()
        assert st == 0
        out.append((costs.cpu().numpy(), g.cpu().numpy()))
    assert np.isfinite(out[0][0]).all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank)
    _check("f32", out[1][0], out[1][1].astype(np.float64), rc, rg, mask, labels, ll, blank, what="0xFF workspace")


def test_invalid_arguments():
    m = _ar()
    N, T, U, A, blank = 2, 4, 3, 7, 0
    tl, ll = np.array([4, 3], np.int32), np.array([2, 1], np.int32)
    lo, hi = np.array([[0, 1], [1, -1]], np.int32), np.array([[2, 3], [2, -1]], np.int32)
    x, labels, tl, ll, lo, hi, _ = _problem("inv", "f32", N, T, U, A, (tl, ll), (lo, hi), blank=blank)
    xd = torch.nan_to_num(x.to(DEV))
    st, c, _ = call(xd, labels, tl, ll, lo, hi, blank, "one")
    assert st == 0 and np.isfinite(c).all()
    # NULL windows
    for null in (("lo",), ("hi",), ("lo", "hi")):
        for form in ("one", "score", "host"):
            st, _, _ = call(xd, labels, tl, ll, lo, hi, blank, form, null=null)
            assert st == 2, (null, form)
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed
    st, c, _ = call(xd, labels, np.array([T + 1, 3], np.int32), ll, lo, hi, blank, "host")
    assert st == 2
    st, c, _ = call(xd, labels, np.array([0, 3], np.int32), ll, lo, hi, blank, "host")
    assert st == 2
    st, c, g = call(xd, labels, tl, np.array([U, 1], np.int32), lo, hi, blank, "one")
    assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
    st, c, g = call(xd, labels, tl, np.array([-1, 1], np.int32), lo, hi, blank, "one")
    assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
    for b in (A, -1):
        for form in ("one", "score"):
            st, _, _ = call(xd, labels, tl, ll, lo, hi, b, form)
            assert st == 2
    # maxU past the limit, maxT maxU >= 2^25 and 2^32 rows are refused before anything is touched
    xb = torch.zeros((1, 1, 4097, 3), device=DEV)
    z = np.zeros((1, 4096), np.int32)
    st, _, _ = call(xb, z, np.array([1], np.int32), np.array([0], np.int32), z, z, 0, "one")
    assert st == 2
    lib = m.lib()
    lab, ttl, tll, tlo, thi = dev(labels, tl, ll, lo, hi)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    costs = torch.zeros(N, device=DEV)
    ptrs = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), tlo.data_ptr(), thi.data_ptr())
    for T2, U2, N2 in ((1 << 13, 4096, N), (1 << 12, 16, 1 << 16)):
        assert lib.compute_rnnt_loss_ar(xd.data_ptr(), None, *ptrs, A, N2, costs.data_ptr(), ws.data_ptr(),
                                        options(T2, U2, blank), 0) == 2
    assert lib.compute_rnnt_loss_ar(xd.data_ptr(), None, *ptrs, (1 << 23) + 1, N, costs.data_ptr(), ws.data_ptr(),
                                    options(T, U, blank), 0) == 2
    # dtype codes, the workspace query, NULL pointers, the CPU location
    n = C.c_size_t(0)
    assert lib.get_workspace_size_ar(4, 3, 1, 4, C.byref(n)) == 2
    assert lib.get_workspace_size_ar(4, 3, 1, -1, C.byref(n)) == 2
    assert lib.get_workspace_size_ar(0, 3, 1, 0, C.byref(n)) == 2
    assert lib.get_workspace_size_ar(4, 3, 1, 0, None) == 2
    assert lib.get_workspace_size_ar(4, 3, 1, 0, C.byref(n)) == 0 and n.value > 0
    for code in (4, -1):
        assert lib.compute_rnnt_loss_ar(xd.data_ptr(), None, *ptrs, A, N, costs.data_ptr(), ws.data_ptr(),
                                        options(T, U, blank), code) == 2, code
    assert lib.compute_rnnt_loss_ar(None, None, *ptrs, A, N, costs.data_ptr(), ws.data_ptr(), options(T, U, blank), 0) == 2
    assert lib.compute_rnnt_loss_ar(xd.data_ptr(), None, *ptrs, A, N, costs.data_ptr(), None, options(T, U, blank), 0) == 2
    assert lib.compute_rnnt_loss_ar_fwd(xd.data_ptr(), *ptrs[:3], None, ptrs[4], A, N, costs.data_ptr(), ws.data_ptr(),
                                        options(T, U, blank), 0, 1) == 2
    assert lib.compute_rnnt_loss_ar_bwd(xd.data_ptr(), None, None, A, N, ws.data_ptr(), options(T, U, blank), 0) == 2
    cpu = options(T, U, blank)
    cpu.loc = 0
    assert lib.compute_rnnt_loss_ar(xd.data_ptr(), None, *ptrs, A, N, costs.data_ptr(), ws.data_ptr(), cpu, 0) == 2
    # gradients that overlap the activations without being them
    buf = torch.zeros(2 * xd.numel(), device=DEV)
    a = buf[:xd.numel()].view(xd.shape).copy_(xd)
    st, _, _ = call(a, labels, tl, ll, lo, hi, blank, "one", grads=buf[4:4 + xd.numel()].view(xd.shape))
    assert st == 2


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_non_finite_inputs(dtype):
    """NaN, +inf or an all -inf row inside the band: that sample only.  The same outside the band: nothing.  A -inf blank or
    label logit is a limit: finite cost while a path is left, +inf when none is."""
    N, T, U, A, blank = 9, 5, 3, 11, 6
    rng = np.random.default_rng(5)
    tl, ll = np.full(N, 4, np.int32), np.full(N, 2, np.int32)
    tl[0] = 5
    # label 0 at frames 0..1, label 1 at frames 1..2: the band is u = 0: t <= 1; u = 1: t <= 2; u = 2: t >= 1
    lo, hi = np.tile(np.array([[0, 1]], np.int32), (N, 1)), np.tile(np.array([[1, 2]], np.int32), (N, 1))
    lo[7], hi[7] = (1, 1), (1, 1)                                # a single path
    x, labels, tl, ll, lo, hi, mask = _problem("nf_" + dtype, dtype, N, T, U, A, (tl, ll), (lo, hi), rng=rng, blank=blank)
    band = mask.copy()
    assert band[1, 1, 0] and band[2, 2, 1] and band[3, 1, 1] and band[4, 3, 2] and not band[5, 0, 2] and not band[5, 3, 0]
    assert int(band[7].sum()) == 4 + 2
    inf = float("inf")
    x[1, 1, 0, 3] = float("nan")                                 # a NaN logit inside the band
    x[2, 2, 1, blank] = float("nan")                             # a NaN blank logit
    x[3, 1, 1, 8] = inf                                          # a +inf logit
    x[4, 3, 2, :] = -inf                                         # an all -inf row
    x[5, 0, 2, :] = inf                                          # outside the band (label 1 not before frame 1): nothing
    x[5, 3, 0, :] = -inf                                         # outside the band (label 0 is out by frame 1): nothing
    x[6, 1, 1, blank] = -inf                                     # no blank out of one cell: paths around it remain
    x[6, 0, 0, int(labels[6, 0])] = -inf
    x[7, 1, 1, int(labels[7, 1])] = -inf                         # the only path closed: no path
    x[8, 3, 2, blank] = -inf                                     # the final blank closed: no path
    st, c, g = call(x.to(DEV), labels, tl, ll, lo, hi, blank, "one")
    assert st == 0
    inl = R.in_lattice_mask((N, T, U), tl, ll)
    for b in (1, 2, 3, 4):
        assert np.isnan(c[b]) and np.isnan(g[b][inl[b]]).all(), (b, c)
    for b in (7, 8):
        assert np.isposinf(c[b]) and np.isnan(g[b][inl[b]]).all(), (b, c)
    assert not g[~inl].any()
    keep = [0, 5, 6]
    assert not g[keep][~band[keep]].any()
    # the reference takes the limit at a logit of -200: autograd through -inf is NaN, and e^-200 is far below every bound
    xr = x[keep].float()
    xr[torch.tensor(~band[keep])] = 0.0
    xr = torch.nan_to_num(xr, nan=0.0).clamp(min=-200.0).to(x.dtype)
    rc, rg = _reference(xr, labels[keep], tl[keep], ll[keep], lo[keep], hi[keep], blank)
    assert np.isfinite(rc).all()
    _check(dtype, c[keep], g[keep], rc, rg, band[keep], labels[keep], ll[keep], blank, what="limits")


@pytest.mark.parametrize("dtype,U", [("f32", 5), ("f64", 5), ("f32", 70)])
def test_infeasible_windows_beside_healthy_samples(dtype, U):
    """An empty window, windows that cannot be ordered and a window wholly past T_b: +inf, NaN on the sample's in-lattice rows
    (none of them is read), zeros on its padding; the others are computed.  The module refuses the batch under validate=True
    and passes it on under validate=False."""
    N, T, A, blank = 4, 12, 9, 2
    tl, ll = np.array([T, 9, 6, 8], np.int32), np.array([U - 1, 3, 2, 2], np.int32)
    rng = np.random.default_rng(U)
    lo, hi, _ = R.windows(rng, tl, ll, U)
    lo[1, :3], hi[1, :3] = (0, 5, 2), (9, 4, 9)                  # an empty window
    lo[2, :2], hi[2, :2] = (3, 0), (5, 2)                        # lo_0 > hi_1
    lo[3, :2], hi[3, :2] = (0, 8), (7, 11)                       # wholly past T_3 = 8
    x, labels, tl, ll, lo, hi, mask = _problem("infeasible_" + dtype, dtype, N, T, U, A, (tl, ll), (lo, hi), rng=rng,
                                               blank=blank)
    assert torch.isnan(x[1:]).all()                              # (no band: every row of the three samples is NaN)
    st, c, g = call(x.to(DEV), labels, tl, ll, lo, hi, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank)
    assert np.isposinf(rc[1:]).all() and np.isfinite(rc[0])
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what="infeasible")
    st, c2, _ = call(x.to(DEV), labels, tl, ll, lo, hi, blank, "host")
    assert st == 0 and np.array_equal(c, c2)                     # (+inf is no invalid-arguments marker)
    from warprnnt_pytorch.ar import AlignmentRestrictedRNNTLoss, rnnt_loss_ar
    xd = torch.nan_to_num(x).to(DEV)
    with pytest.raises(ValueError, match=r"sample 1 has no path: label 1 needs a frame in \[5, 4\]"):
        AlignmentRestrictedRNNTLoss(blank=blank, reduction="none")(xd, *dev(labels, tl, ll, lo, hi))
    out = rnnt_loss_ar(xd, *dev(labels, tl, ll, lo, hi), blank=blank, reduction="none", validate=False)
    assert torch.isfinite(out[0]) and torch.isposinf(out[1:]).all()


def test_label_equal_to_the_blank():
    """Legal: the column carries both edges' posteriors."""
    N, T, U, A, blank = 3, 6, 4, 9, 4
    rng = np.random.default_rng(21)
    tl, ll = np.array([6, 5, 6], np.int32), np.array([3, 2, 1], np.int32)
    lo, hi, _ = R.windows(rng, tl, ll, U)
    x, labels, tl, ll, lo, hi, mask = _problem("lab", "f32", N, T, U, A, (tl, ll), (lo, hi), rng=rng, blank=blank)
    labels[0, 1] = blank
    labels[1, 0] = blank
    labels[1, 1] = blank
    labels[2, 2] = blank               # behind L_2 = 1: never looked at
    st, c, g = call(x.to(DEV), labels, tl, ll, lo, hi, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank)
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, what="label on the blank")
    from warprnnt_pytorch.ar import rnnt_loss_ar
    out = rnnt_loss_ar(torch.nan_to_num(x).to(DEV), *dev(labels, tl, ll, lo, hi), blank=blank, reduction="none")
    assert np.allclose(out.cpu().numpy(), rc, rtol=1e-5)


def test_closed_form_fully_pinned():
    """Every label pinned: cost = -(the one path's weights), in fp64; both lattice forms."""
    rng = np.random.default_rng(4)
    for L, T in ((1, 3), (5, 4), (63, 9), (64, 9), (100, 7)):
        A, blank = 6, 1
        x = torch.tensor(rng.standard_normal((1, T, L + 1, A)), dtype=torch.float64)
        labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
        a = np.sort(rng.integers(0, T, size=(1, L))).astype(np.int32)
        st, c, _ = call(x.to(DEV), labels, np.array([T], np.int32), np.array([L], np.int32), a, a, blank, "score")
        lp = torch.log_softmax(x[0], -1).numpy()
        want, u = 0.0, 0
        for t in range(T):
            while u < L and a[0, u] == t:
                want += lp[t, u, labels[0, u]]
                u += 1
            want += lp[t, u, blank]
        assert st == 0 and abs(c[0] + want) < 1e-9 * max(1.0, abs(want)), (L, c, want)


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_reductions(reduction):
    from warprnnt_pytorch.ar import AlignmentRestrictedRNNTLoss
    N, T, U, A, blank = 3, 6, 4, 11, 10
    rng = np.random.default_rng(3)
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 3], np.int32)
    lo, hi, _ = R.windows(rng, tl, ll, U)
    x, labels, tl, ll, lo, hi, mask = _problem("ag", "f32", N, T, U, A, (tl, ll), (lo, hi), rng=rng, blank=blank)
    x = torch.nan_to_num(x)
    xd = x.to(DEV).requires_grad_()
    loss = AlignmentRestrictedRNNTLoss(blank=blank, reduction=reduction)(xd, *dev(labels, tl, ll, lo, hi))
    go = torch.tensor([0.7, -1.3, 2.0][:loss.numel()], device=DEV).view(loss.shape)
    (loss * go).sum().backward()
    w = go.detach().cpu().numpy().reshape(-1)
    w = np.broadcast_to(w, (N,)) / (N if reduction == "mean" else 1)
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank, weights=w)
    want = {"none": rc, "sum": rc.sum(keepdims=True), "mean": rc.mean(keepdims=True)}[reduction]
    assert np.allclose(loss.detach().cpu().numpy(), want, rtol=1e-5)
    got = xd.grad.double().cpu().numpy()
    assert not got[~mask].any()
    O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank)[mask], torch.float32)


def test_gradcheck_fp64():
    from warprnnt_pytorch.ar import rnnt_loss_ar
    N, T, U, A, blank = 2, 4, 3, 6, 2
    rng = np.random.default_rng(2)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    lo, hi = np.array([[0, 1], [1, -1]], np.int32), np.array([[2, 3], [2, -1]], np.int32)
    lab, ttl, tll, tlo, thi = dev(labels, np.array([4, 3], np.int32), np.array([2, 1], np.int32), lo, hi)
    x = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda z: rnnt_loss_ar(z, lab, ttl, tll, tlo, thi, blank, "none"), (x,), eps=1e-6,
                                    atol=1e-6, nondet_tol=1e-12)


def test_cpu_tensors_are_refused():
    from warprnnt_pytorch.ar import rnnt_loss_ar
    x = torch.zeros(1, 2, 2, 5)
    i32 = dict(dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        rnnt_loss_ar(x, torch.ones(1, 1, **i32), torch.tensor([2], **i32), torch.tensor([1], **i32), torch.zeros(1, 1, **i32),
                     torch.ones(1, 1, **i32), blank=4)


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch), replayed on new logits."""
    from warprnnt_pytorch.ar import rnnt_loss_ar
    N, T, U, A, blank = 3, 8, 5, 33, 32
    rng = np.random.default_rng(11)
    tl, ll = np.array([8, 6, 4], np.int32), np.array([4, 0, 4], np.int32)
    labels = rng.integers(0, A - 1, size=(N, U - 1)).astype(np.int32)
    lo, hi, _ = R.windows(rng, tl, ll, U)
    lab, ttl, tll, tlo, thi = dev(labels, tl, ll, lo, hi)
    static_x = torch.zeros((N, T, U, A), device=DEV, requires_grad=True)
    m = _ar()
    m.lib()
    m.workspace_bytes(T, U, N, 0)

    def step():
        static_x.grad = None
        loss = rnnt_loss_ar(static_x, lab, ttl, tll, tlo, thi, blank, "sum", validate=False)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    static_x.grad = None
    with torch.cuda.graph(graph):
        loss = rnnt_loss_ar(static_x, lab, ttl, tll, tlo, thi, blank, "sum", validate=False)
        loss.backward()
    grad = static_x.grad
    mask = R.band_mask((N, T, U), tl, ll, lo, hi)
    for seed in (1, 2):
        xn = np.random.default_rng(seed).standard_normal((N, T, U, A)).astype(np.float32)
        with torch.no_grad():
            static_x.copy_(torch.tensor(xn))
        graph.replay()
        torch.cuda.synchronize()
        rc, rg = R.ar_autograd(xn, labels, tl, ll, lo, hi, blank)
        assert abs(loss.item() - rc.sum()) < 1e-5 * rc.sum()
        got = grad.double().cpu().numpy()
        assert not got[~mask].any()
        O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank)[mask], torch.float32, what="replay %d" % seed)


# ----------------------------------------------------------------------------- long utterances: the per-diagonal offsets
@pytest.mark.parametrize("U,A", [(301, 50), (33, 8)])
def test_long_utterance(U, A):
    """T = 1500, fp32, windows of +-20 frames around an alignment spread over the utterance: the block form's per-diagonal
    offsets (U = 301, the second sample short) and the wave form's per-chunk ones (U = 33, 191 re-centrings)."""
    N, T, blank = 2, 1500, A - 1
    rng = np.random.default_rng(7)
    tl, ll = np.array([T, 100], np.int32), np.array([U - 1, 30], np.int32)
    lo, hi = np.full((N, U - 1), -1, np.int32), np.full((N, U - 1), -1, np.int32)
    for b in range(N):
        a = np.sort(rng.integers(0, tl[b], size=ll[b]))
        lo[b, :ll[b]], hi[b, :ll[b]] = a - 20, a + 20
    x, labels, tl, ll, lo, hi, mask = _problem("long", "f32", N, T, U, A, (tl, ll), (lo, hi), rng=rng, scale=1.0, blank=blank)
    st, c, g = call(x.to(DEV), labels, tl, ll, lo, hi, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, lo, hi, blank)
    assert np.isfinite(rc).all()
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, what="long U = %d" % U)


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_in_place_past_2_31_elements():
    """bf16 in place, N T U A > 2^31 elements: the last sample's band rows lie past element 2^31.  The reference is taken over
    the few in-lattice rows only."""
    N, T, U, A, blank = 5, 64, 65, 130001, 70000
    E = N * T * U * A
    assert E > 2 ** 31 and 4 * T * U * A > 2 ** 31 - 3 * T * U * A
    need = 2 * E + (1 << 30)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        print("SKIPPED: %d bytes of device memory free, the tensor past 2^31 elements needs %d" % (free, need))
        pytest.skip("device memory is short")
    tl, ll = np.array([1, 2, 3, 2, 4], np.int32), np.array([0, 1, 2, 1, 3], np.int32)
    rng = np.random.default_rng(13)
    labels = rng.integers(4, 60000, size=(N, U - 1)).astype(np.int32)
    lo, hi = np.full((N, U - 1), -1, np.int32), np.full((N, U - 1), -1, np.int32)
    lo[1, 0], hi[1, 0] = 1, 1
    lo[2, :2], hi[2, :2] = (0, 1), (1, 2)
    lo[3, 0], hi[3, 0] = -4, 9
    lo[4, :3], hi[4, :3] = (0, 1, 2), (1, 3, 3)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((N, T, U, A), generator=g, device=DEV, dtype=torch.bfloat16)
    small = torch.zeros((N, 4, 4, A), dtype=torch.float64)
    for b in range(N):
        small[b, :tl[b], :ll[b] + 1] = x[b, :tl[b], :ll[b] + 1].double().cpu()
    st, c, _ = call(x, labels, tl, ll, lo, hi, blank, "inplace")
    assert st == 0
    rc, rg = R.ar_autograd(small.numpy(), labels[:, :3], tl, ll, lo[:, :3], hi[:, :3], blank)
    assert np.isfinite(rc).all() and np.allclose(c, rc, rtol=1e-5, atol=1e-5), (c, rc)
    band = R.band_mask((N, 4, 4), tl, ll, lo, hi)
    assert band[4].sum() < (tl[4] * (ll[4] + 1)) and band[4, 3, 3]
    for b in range(N):
        assert x[b, tl[b]:].count_nonzero().item() == 0
        assert x[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
        got = x[b, :4, :4].double().cpu().numpy()
        assert not got[~band[b]].any()
        ref = rg[b]
        O.assert_grads(got[band[b]], ref[band[b]], np.maximum(np.abs(ref), np.abs(ref).sum(-1, keepdims=True))[band[b]],
                       torch.bfloat16, what="sample %d" % b)
