"""-m gpu: the delay-penalized RNN-T loss and the expected emission frames (include/rnnt_delay.h, libwarprnnt_delay.so).

Every case of tests/delay_forms.py runs through the one-call C-ABI entry under torch.profiler at delay_penalty = 0.3 with
gradients and emit_frames: exactly the kernels its release rules predict run, stage by stage.  Costs and gradients go through
gpu_support.check against the fp64 autograd reference of tests/delay_ref.py: costs at COST_TOL, gradients per element at
oracle.grad_bound with mag = |ref| and, for the blank and label columns, the row's |ref| sum.  emit_frames: per element
|err| <= r ref + a T_b (T_b - 1) / 2 with (r, a) oracle.py's relative and absolute constants of the lattice type -- the sum
over t of t times the project's bound on a posterior.  NaN in every padding row (never read), gradient and emit_frames
buffers that start as NaN.  The reference takes the penalty the library sees: the value of the C-ABI's float.

A negative control compares the result at 0.5 with the reference at 0 and must fail.  Then a penalty of 0 against RNNTLoss,
monotonicity in the penalty, the call forms, bit-identical reruns and workspaces, the invalid arguments, the non-finite cases
of the header, a label on the blank column, the closed form at T_b = 1, the autograd module, a HIP-graph capture, two long
utterances and one bf16 tensor past 2^31 elements."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import delay_forms as F
from tests import delay_ref as R
from tests import gpu_support as G
from tests.gpu_support import (CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check,
                               dev, options, place, profiled, stages_seen)

pytestmark = pytest.mark.gpu
PEN = R.f32_penalty(0.3)


def _delay():
    from warprnnt_pytorch import delay
    return delay


def _problem(name, dtype, N, T, U, A, lengths, rng=None, scale=2.0, blank=None):
    """Logits with NaN in every padding row, labels over all of [0, A) but the blank, the lengths and the in-lattice mask."""
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = np.asarray(lengths[0], np.int32), np.asarray(lengths[1], np.int32)
    allowed = [c for c in range(A) if c != blank] or [0]
    labels = rng.choice(allowed, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * scale, dtype=torch.float32).to(TORCH[dtype])
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    x[torch.tensor(~mask)] = float("nan")
    return x, labels, tl, ll, mask


def _table_problem(name, dtype, N, T, U, A, blank, seed=None):
    rng = np.random.default_rng(zlib.crc32(name.encode()) if seed is None else seed)
    tl, ll = F.lengths(dict(N=N, T=T, U=U), rng)
    return _problem(name, dtype, N, T, U, A, (tl, ll), rng=rng, blank=blank)


def _frames_buffer(x):
    """(N, U - 1) of the costs' type, NaN throughout."""
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    return torch.full((x.shape[0], x.shape[2] - 1), float("nan"), dtype=cdt, device=DEV)


def call(x, labels, tl, ll, blank=0, penalty=PEN, form="one", scale=None, grads=None, stream=None, emit=True, prepare=1, ws=None):
    """One C-ABI call form -> (status, costs, grads or None, emit_frames or None).  form: one | two | inplace | score | host.
    emit: True (a NaN buffer of this call's own), a tensor, or False / None (NULL)."""
    m = _delay()
    N, T, U, A = x.shape
    code = CODE[NAME[x.dtype]]
    pad = np.zeros((N, 1), np.int32)
    lab, ttl, tll = dev(labels if labels.size else pad, tl, ll)
    opt = options(T, U, blank, stream)
    lib = m.lib()
    fr = _frames_buffer(x) if emit is True else (emit if torch.is_tensor(emit) else None)
    ep = fr.data_ptr() if fr is not None and fr.numel() else None
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    st, c, g = call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_rnnt_loss_delay(x.data_ptr(), penalty, gp, *lens, costs, ep, ws, opt, code),
        lambda costs, ws: lib.compute_rnnt_loss_delay_fwd(x.data_ptr(), penalty, *lens, costs, ep, ws, opt, code, prepare),
        lambda gp, sc, ws: lib.compute_rnnt_loss_delay_bwd(x.data_ptr(), gp, sc, A, N, ws, opt, code),
        m.workspace_bytes(T, U, N, code), scale, grads, stream, ws)
    torch.cuda.synchronize()
    return st, c, g, (None if fr is None else fr.double().cpu().numpy())


def _clean(x):
    return torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()


def _reference(x, labels, tl, ll, blank=0, penalty=PEN, weights=None):
    return R.delay_autograd(_clean(x), labels, tl, ll, blank, penalty, weights)


def _emit_reference(x, labels, tl, ll, blank=0, penalty=PEN):
    return R.emit_frames_ref(_clean(x), labels, tl, ll, blank, penalty)


def _reference_all(x, labels, tl, ll, blank=0, penalty=PEN):
    """(costs, gradients, emit_frames) of one pass of the reference."""
    return R.delay_all(_clean(x), labels, tl, ll, blank, penalty)


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


def _check_emit(dtype, got, ref, tl, ll, what=""):
    """Per element |err| <= r ref + a T_b (T_b - 1) / 2, (r, a) of the lattice type (oracle.py); exact zeros behind a
    sample's labels.  Returns the worst err / bound."""
    lat = "fp64" if dtype == "f64" else "fp32"
    r, a = O._REL[lat], O._ABS[lat]
    tl = np.asarray(tl, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    behind = np.arange(ref.shape[1])[None, :] >= np.asarray(ll)[:, None]
    assert not got[behind].any(), (what, "exact zeros behind the labels")          # (NaN counts as nonzero)
    bound = r * np.abs(ref) + a * (tl * (tl - 1) / 2)[:, None]
    err = np.abs(got - ref)
    live = ~behind
    assert np.isfinite(got[live]).all(), (what, got)
    assert not err[live & (bound == 0)].any(), (what, "T_b = 1: exact zeros")
    ratio = err[live & (bound > 0)] / bound[live & (bound > 0)]
    worst = float(ratio.max()) if ratio.size else 0.0
    print(what, "max emit_frames error / bound = %.4f" % worst)
    assert worst <= 1.0, (what, worst, got, ref)
    return worst


# ----------------------------------------------------------------------------- every form of tests/delay_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_delay_form(name):
    case = F.CASES[name]
    cus = G.cus()
    N, T, U, A, dtype, blank = case["N"], case["T"], case["U"], case["A"], case["dtype"], case["blank"]
    x, labels, tl, ll, mask = _table_problem(name, dtype, N, T, U, A, blank)
    off = case.get("off", 0)
    xv = place(x.to(DEV), off, x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    (st, c, g, fr), names = profiled(lambda: call(xv, labels, tl, ll, blank, PEN, "one", grads=gv))
    if st == 0 and not names:                        # (a profiler session now and then records no device event at all:
        gv.fill_(float("nan"))                       #  one more session, judged as the first would have been)
        (st, c, g, fr), names = profiled(lambda: call(xv, labels, tl, ll, blank, PEN, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, cus))
    rc, rg, re = _reference_all(x, labels, tl, ll, blank)
    assert np.isfinite(rc).all()
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what=name)
    _check_emit(dtype, fr, re, tl, ll, what=name)


def test_every_delay_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_negative_control_the_unpenalized_loss_is_refused(dtype):
    """The result at delay_penalty = 0.5 against the reference at 0 must fail, for costs, gradients and emit_frames: the
    checks cannot pass on the plain loss.  Every sample has 1 <= L_b and T_b >= 3."""
    N, T, U, A, blank = 4, 9, 7, 12, 11
    tl, ll = np.array([9, 5, 7, 3], np.int32), np.array([6, 2, 1, 2], np.int32)
    x, labels, tl, ll, mask = _problem("neg_" + dtype, dtype, N, T, U, A, (tl, ll), blank=blank)
    st, c, g, fr = call(x.to(DEV), labels, tl, ll, blank, 0.5, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, blank, 0.5)
    re = _emit_reference(x, labels, tl, ll, blank, 0.5)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what="penalized")
    _check_emit(dtype, fr, re, tl, ll, what="penalized")
    pc, pg = _reference(x, labels, tl, ll, blank, 0.0)
    pe = _emit_reference(x, labels, tl, ll, blank, 0.0)
    assert (np.abs(pc - rc) >= 100 * COST_TOL[dtype]).all(), (pc, rc)                # (on the CPU: the two references differ)
    assert np.abs(pg - rg).max() >= 1e-2 and (np.abs(pe - re).max(1) >= 1e-2).all()
    with pytest.raises(AssertionError):
        _check(dtype, c, None, pc, pg, mask, labels, ll, blank, what="plain costs")
    with pytest.raises(AssertionError):
        _check(dtype, rc, g, rc, pg, mask, labels, ll, blank, what="plain gradients")
    with pytest.raises(AssertionError):
        _check_emit(dtype, fr, pe, tl, ll, what="plain emit_frames")


def test_penalty_zero_is_rnntloss():
    """delay_penalty = 0 against RNNTLoss on the same raw logits, with labels, fp64, on the GPU."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.delay import rnnt_loss_delay
    N, T, U, A, blank = 4, 12, 5, 37, 9
    rng = np.random.default_rng(17)
    tl, ll = np.array([12, 1, 7, 9], np.int32), np.array([4, 2, 0, 3], np.int32)
    labels = rng.choice([c for c in range(A) if c != blank], size=(N, U - 1)).astype(np.int32)
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * 2, dtype=torch.float64, device=DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    xa = x.clone().requires_grad_()
    la = rnnt_loss_delay(xa, lab, ttl, tll, blank, 0.0, "none", validate=False)
    la.sum().backward()
    xb = x.clone().requires_grad_()
    lb = RNNTLoss(blank=blank, reduction="none", validate=False)(xb, lab, ttl, tll)
    lb.sum().backward()
    assert torch.allclose(la, lb, rtol=1e-9, atol=0), (la, lb)
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    ga, gb = xa.grad.cpu().numpy(), xb.grad.cpu().numpy()
    assert not ga[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, ll, blank)[mask], torch.float64, what="cross-check")


@pytest.mark.parametrize("U", [6, 70])
def test_emit_frames_fall_as_the_penalty_rises(U):
    """sum_u emit_frames[b, u] at delay_penalty = -0.5, 0, 0.5 is strictly decreasing for every sample with more than one
    path (T_b >= 2 and L_b >= 1): its derivative is minus the variance of the total emission time.  The others stay put."""
    from warprnnt_pytorch.delay import expected_emit_frames
    N, T, A, blank = 6, 11, 9, 0
    x, labels, tl, ll, _ = _table_problem("monotone", "f64", N, T, U, A, blank, seed=U)
    xd = torch.nan_to_num(x).to(DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    sums, costs = [], []
    for pen in (-0.5, 0.0, 0.5):
        c, fr = expected_emit_frames(xd, lab, ttl, tll, blank, pen)
        assert fr.shape == (N, U - 1) and fr.dtype == torch.float64 and c.shape == (N,)
        sums.append(fr.sum(1).cpu().numpy())
        costs.append(c.cpu().numpy())
        rc, _ = _reference(xd, labels, tl, ll, blank, pen)
        assert np.allclose(costs[-1], rc, rtol=1e-9, atol=1e-9)
    many = (tl >= 2) & (ll >= 1)
    assert many.any() and (~many).any()
    assert (sums[0][many] > sums[1][many]).all() and (sums[1][many] > sums[2][many]).all(), sums
    assert np.array_equal(sums[0][~many], sums[1][~many]) and np.array_equal(sums[1][~many], sums[2][~many])


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("dtype,U", [("f32", 9), ("bf16", 9), ("f32", 66), ("f64", 70)])
def test_call_forms_agree(dtype, U):
    N, T, A, blank = 5, 11, 130, 129
    x, labels, tl, ll, mask = _table_problem("forms_" + dtype, dtype, N, T, U, A, blank, seed=U)
    xd = x.to(DEV)
    st, c1, g1, e1 = call(xd, labels, tl, ll, blank, PEN, "one")
    assert st == 0
    _check_emit(dtype, e1, _emit_reference(x, labels, tl, ll, blank), tl, ll, what="one call")
    # without emit_frames: the same costs and gradients
    st, c0, g0, e0 = call(xd, labels, tl, ll, blank, PEN, "one", emit=False)
    assert st == 0 and e0 is None and np.array_equal(c1, c0) and np.array_equal(g1, g0)
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    for emit in (True, False):
        st, c2, g2, e2 = call(xd, labels, tl, ll, blank, PEN, "two", scale=scale, emit=emit)
        assert st == 0 and np.array_equal(c1, c2) and (not emit or np.array_equal(e1, e2))
        rc, rg = _reference(x, labels, tl, ll, blank, weights=scale)
        _check(dtype, c2, g2, rc, rg, mask, labels, ll, blank, what="two-phase")
        st, c2b, g2b, _ = call(xd, labels, tl, ll, blank, PEN, "two", scale=np.ones(N), emit=emit)
        assert st == 0 and np.array_equal(c1, c2b) and np.array_equal(g2b, g1)            # bit for bit at scale 1
        xi = xd.clone()
        st, c3, g3, e3 = call(xi, labels, tl, ll, blank, PEN, "inplace", emit=emit)
        assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1) and (not emit or np.array_equal(e1, e3))
        st, c4, _, e4 = call(xd, labels, tl, ll, blank, PEN, "score", emit=emit)
        assert st == 0 and np.array_equal(c1, c4) and (not emit or np.array_equal(e1, e4))
        st, c5, g5, e5 = call(xd, labels, tl, ll, blank, PEN, "host", grads=torch.full_like(xd, float("nan")), emit=emit)
        assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5) and np.array_equal(g5, g1)
        assert not emit or np.array_equal(e1, e5)
    # _fwd with prepare_backward = 0 and emit_frames: the same frames
    m = _delay()
    code = CODE[dtype]
    lab, ttl, tll = dev(labels, tl, ll)
    fr = _frames_buffer(xd)
    costs = torch.full((N,), float("nan"), dtype=fr.dtype, device=DEV)
    ws = torch.empty(m.workspace_bytes(T, U, N, code), dtype=torch.uint8, device=DEV)
    st = m.lib().compute_rnnt_loss_delay_fwd(xd.data_ptr(), PEN, lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N,
                                             costs.data_ptr(), fr.data_ptr(), ws.data_ptr(), options(T, U, blank), code, 0)
    torch.cuda.synchronize()
    assert st == 0 and np.array_equal(fr.double().cpu().numpy(), e1) and np.array_equal(costs.cpu().numpy(), c1)
    # a second run: identical bits
    st, c6, g6, e6 = call(xd, labels, tl, ll, blank, PEN, "one")
    assert st == 0 and np.array_equal(c1, c6) and np.array_equal(g1, g6) and np.array_equal(e1, e6)


@pytest.mark.parametrize("U", [6, 70])
def test_workspace_contents_do_not_matter(U):
    """A workspace full of 0xFF bytes (NaN as values, -1 as flags) gives the bits a zeroed one gives: nothing an earlier call
    left reaches arithmetic."""
    m = _delay()
    N, T, A, blank = 5, 13, 19, 3
    x, labels, tl, ll, mask = _table_problem("ws", "f32", N, T, U, A, blank, seed=U)
    xd = x.to(DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    out = []
    for fill in (0, 255):
        ws = torch.full((m.workspace_bytes(T, U, N, 0),), fill, dtype=torch.uint8, device=DEV)
        costs = torch.full((N,), float("nan"), device=DEV)
        g = torch.full_like(xd, float("nan"))
        fr = _frames_buffer(xd)
        st = m.lib().compute_rnnt_loss_delay(xd.data_ptr(), PEN, g.data_ptr(), lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(),
                                             A, N, costs.data_ptr(), fr.data_ptr(), ws.data_ptr(), options(T, U, blank), 0)
        torch.cuda.synchronize()
        assert st == 0
        out.append((costs.cpu().numpy(), g.cpu().numpy(), fr.cpu().numpy()))
    assert np.isfinite(out[0][0]).all()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    rc, rg = _reference(x, labels, tl, ll, blank)
    _check("f32", out[1][0], out[1][1].astype(np.float64), rc, rg, mask, labels, ll, blank, what="0xFF workspace")
    _check_emit("f32", out[1][2].astype(np.float64), _emit_reference(x, labels, tl, ll, blank), tl, ll, what="0xFF workspace")


def test_invalid_arguments():
    m = _delay()
    N, T, U, A, blank = 2, 4, 3, 7, 0
    tl, ll = np.array([4, 3], np.int32), np.array([2, 1], np.int32)
    x, labels, tl, ll, _ = _problem("inv", "f32", N, T, U, A, (tl, ll), blank=blank)
    xd = torch.nan_to_num(x.to(DEV))
    st, c, _, fr = call(xd, labels, tl, ll, blank, PEN, "one")
    assert st == 0 and np.isfinite(c).all() and np.isfinite(fr).all()
    # a penalty that is not finite; negative ones are accepted
    for bad in (float("nan"), float("inf"), -float("inf")):
        for form in ("one", "score", "host"):
            st, _, _, _ = call(xd, labels, tl, ll, blank, bad, form)
            assert st == 2, (bad, form)
    st, c, _, _ = call(xd, labels, tl, ll, blank, -3.0, "one")
    assert st == 0 and np.isfinite(c).all()
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed, the
    # gradients and emit_frames of the bad one are zero
    st, c, _, _ = call(xd, labels, np.array([T + 1, 3], np.int32), ll, blank, PEN, "host")
    assert st == 2
    st, c, _, _ = call(xd, labels, np.array([0, 3], np.int32), ll, blank, PEN, "host")
    assert st == 2
    for bad_ll in (U, -1):
        st, c, g, fr = call(xd, labels, tl, np.array([bad_ll, 1], np.int32), blank, PEN, "one")
        assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
        assert not fr[0].any() and fr[1, 0] > 0 and fr[1, 1] == 0
    for b in (A, -1):
        for form in ("one", "score"):
            st, _, _, _ = call(xd, labels, tl, ll, b, PEN, form)
            assert st == 2
    # maxU past the limit, maxT maxU >= 2^25 and 2^32 rows are refused before anything is touched
    xb = torch.zeros((1, 1, 4097, 3), device=DEV)
    st, _, _, _ = call(xb, np.zeros((1, 4096), np.int32), np.array([1], np.int32), np.array([0], np.int32), 0, PEN, "one")
    assert st == 2
    lib = m.lib()
    lab, ttl, tll = dev(labels, tl, ll)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    costs = torch.zeros(N, device=DEV)
    fr = _frames_buffer(xd)
    ptrs = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr())
    for T2, U2, N2 in ((1 << 13, 4096, N), (1 << 12, 16, 1 << 16)):
        assert lib.compute_rnnt_loss_delay(xd.data_ptr(), PEN, None, *ptrs, A, N2, costs.data_ptr(), None, ws.data_ptr(),
                                           options(T2, U2, blank), 0) == 2
    assert lib.compute_rnnt_loss_delay(xd.data_ptr(), PEN, None, *ptrs, (1 << 23) + 1, N, costs.data_ptr(), None, ws.data_ptr(),
                                       options(T, U, blank), 0) == 2
    # dtype codes, the workspace query, NULL pointers, the CPU location
    n = C.c_size_t(0)
    assert lib.get_workspace_size_delay(4, 3, 1, 4, C.byref(n)) == 2
    assert lib.get_workspace_size_delay(4, 3, 1, -1, C.byref(n)) == 2
    assert lib.get_workspace_size_delay(0, 3, 1, 0, C.byref(n)) == 2
    assert lib.get_workspace_size_delay(4, 3, 1, 0, None) == 2
    assert lib.get_workspace_size_delay(4, 3, 1, 0, C.byref(n)) == 0 and n.value > 0
    one = lambda **kw: lib.compute_rnnt_loss_delay(                                                          # noqa: E731
        kw.get("acts", xd.data_ptr()), PEN, kw.get("grads"), *ptrs, A, N, costs.data_ptr(), kw.get("emit", fr.data_ptr()),
        kw.get("ws", ws.data_ptr()), kw.get("opt", options(T, U, blank)), kw.get("code", 0))
    assert one() == 0
    for code in (4, -1):
        assert one(code=code) == 2, code
    assert one(acts=None) == 2 and one(ws=None) == 2
    assert lib.compute_rnnt_loss_delay_bwd(xd.data_ptr(), None, None, A, N, ws.data_ptr(), options(T, U, blank), 0) == 2
    cpu = options(T, U, blank)
    cpu.loc = 0
    assert one(opt=cpu) == 2
    # emit_frames inside the activations, the gradients or the workspace, or off its element boundary
    g = torch.zeros_like(xd)
    assert one(grads=g.data_ptr()) == 0
    assert one(emit=xd.data_ptr() + 16) == 2 and one(emit=ws.data_ptr() + 64) == 2 and one(emit=fr.data_ptr() + 2) == 2
    assert one(grads=g.data_ptr(), emit=g.data_ptr() + 32) == 2
    torch.cuda.synchronize()
    # gradients that overlap the activations without being them
    buf = torch.zeros(2 * xd.numel(), device=DEV)
    a = buf[:xd.numel()].view(xd.shape).copy_(xd)
    st, _, _, _ = call(a, labels, tl, ll, blank, PEN, "one", grads=buf[4:4 + xd.numel()].view(xd.shape))
    assert st == 2


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_non_finite_inputs(dtype):
    """NaN, +inf or an all -inf row inside the lattice: that sample only -- NaN cost, NaN gradients on its in-lattice rows,
    NaN emit_frames for u < L_b and exact zeros behind.  A -inf blank or label logit is a limit: finite cost while a path is
    left, +inf (and the same NaNs) when none is."""
    N, T, U, A, blank = 8, 5, 4, 11, 6
    rng = np.random.default_rng(5)
    tl, ll = np.full(N, 4, np.int32), np.full(N, 2, np.int32)
    tl[0] = 5
    ll[6] = 3
    x, labels, tl, ll, mask = _problem("nf_" + dtype, dtype, N, T, U, A, (tl, ll), rng=rng, blank=blank)
    inf = float("inf")
    x[1, 1, 0, 3] = float("nan")                                 # a NaN logit
    x[2, 2, 1, blank] = float("nan")                             # a NaN blank logit
    x[3, 1, 1, 8] = inf                                          # a +inf logit
    x[4, 3, 2, :] = -inf                                         # an all -inf row
    x[5, 1, 1, blank] = -inf                                     # no blank out of one cell: paths around it remain
    x[5, 0, 0, int(labels[5, 0])] = -inf
    x[6, 3, 3, blank] = -inf                                     # the final blank closed: no path
    x[7, :, 1, int(labels[7, 1])] = -inf                         # label 1 can never be emitted: no path
    st, c, g, fr = call(x.to(DEV), labels, tl, ll, blank, PEN, "one")
    assert st == 0
    for b in (1, 2, 3, 4):
        assert np.isnan(c[b]) and np.isnan(g[b][mask[b]]).all(), (b, c)
    for b in (6, 7):
        assert np.isposinf(c[b]) and np.isnan(g[b][mask[b]]).all(), (b, c)
    for b in (1, 2, 3, 4, 6, 7):
        assert np.isnan(fr[b, :ll[b]]).all() and not fr[b, ll[b]:].any(), (b, fr[b])
    assert not g[~mask].any()
    keep = [0, 5]
    # the reference takes the limit at a logit of -200: autograd through -inf is NaN, and e^-200 is far below every bound
    xr = x[keep].float()
    xr[torch.tensor(~mask[keep])] = 0.0
    xr = torch.nan_to_num(xr, nan=0.0).clamp(min=-200.0).to(x.dtype)
    rc, rg = _reference(xr, labels[keep], tl[keep], ll[keep], blank)
    assert np.isfinite(rc).all()
    _check(dtype, c[keep], g[keep], rc, rg, mask[keep], labels[keep], ll[keep], blank, what="limits")
    _check_emit(dtype, fr[keep], _emit_reference(xr, labels[keep], tl[keep], ll[keep], blank), tl[keep], ll[keep], what="limits")


def test_label_equal_to_the_blank():
    """Legal: the column carries both edges' posteriors."""
    N, T, U, A, blank = 3, 6, 4, 9, 4
    tl, ll = np.array([6, 5, 6], np.int32), np.array([3, 2, 1], np.int32)
    x, labels, tl, ll, mask = _problem("lab", "f32", N, T, U, A, (tl, ll), blank=blank)
    labels[0, 1] = blank
    labels[1, 0] = blank
    labels[1, 1] = blank
    labels[2, 2] = blank               # behind L_2 = 1: never looked at
    st, c, g, fr = call(x.to(DEV), labels, tl, ll, blank, PEN, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, blank)
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, what="label on the blank")
    _check_emit("f32", fr, _emit_reference(x, labels, tl, ll, blank), tl, ll, what="label on the blank")


def test_closed_form_single_frame():
    """T_b = 1: every label at frame 0, one path: emit_frames == 0 and cost = -(sum of the path's log-probabilities)
    - delay_penalty * L * 0, whatever the penalty; fp64, both lattice forms."""
    rng = np.random.default_rng(4)
    for L in (1, 5, 63, 64, 100):
        A, blank = 6, 1
        x = torch.tensor(rng.standard_normal((1, 1, L + 1, A)), dtype=torch.float64)
        labels = rng.integers(0, A, size=(1, L)).astype(np.int32)
        lp = torch.log_softmax(x[0, 0], -1).numpy()
        want = -(sum(lp[u, labels[0, u]] for u in range(L)) + lp[L, blank])
        for pen in (0.0, PEN, -2.0):
            st, c, _, fr = call(x.to(DEV), labels, np.array([1], np.int32), np.array([L], np.int32), blank, pen, "score")
            assert st == 0 and abs(c[0] - want) < 1e-9 * max(1.0, abs(want)), (L, pen, c, want)
            assert fr.shape == (1, L) and not fr.any()


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_reductions(reduction):
    from warprnnt_pytorch.delay import DelayPenalizedRNNTLoss
    N, T, U, A, blank = 3, 6, 4, 11, 10
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 3], np.int32)
    x, labels, tl, ll, mask = _problem("ag", "f32", N, T, U, A, (tl, ll), blank=blank)
    x = torch.nan_to_num(x)
    xd = x.to(DEV).requires_grad_()
    loss = DelayPenalizedRNNTLoss(blank=blank, delay_penalty=0.3, reduction=reduction)(xd, *dev(labels, tl, ll))
    go = torch.tensor([0.7, -1.3, 2.0][:loss.numel()], device=DEV).view(loss.shape)
    (loss * go).sum().backward()
    w = go.detach().cpu().numpy().reshape(-1)
    w = np.broadcast_to(w, (N,)) / (N if reduction == "mean" else 1)
    rc, rg = _reference(x, labels, tl, ll, blank, weights=w)
    want = {"none": rc, "sum": rc.sum(keepdims=True), "mean": rc.mean(keepdims=True)}[reduction]
    assert np.allclose(loss.detach().cpu().numpy(), want, rtol=1e-5)
    got = xd.grad.double().cpu().numpy()
    assert not got[~mask].any()
    O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank)[mask], torch.float32)


def test_gradcheck_fp64():
    from warprnnt_pytorch.delay import rnnt_loss_delay
    N, T, U, A, blank = 2, 4, 3, 6, 2
    rng = np.random.default_rng(2)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    lab, ttl, tll = dev(labels, np.array([4, 3], np.int32), np.array([2, 1], np.int32))
    x = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda z: rnnt_loss_delay(z, lab, ttl, tll, blank, 0.3, "none"), (x,), eps=1e-6,
                                    atol=1e-6, nondet_tol=1e-12)


def test_cpu_tensors_are_refused():
    from warprnnt_pytorch.delay import expected_emit_frames, rnnt_loss_delay
    x = torch.zeros(1, 2, 2, 5)
    i32 = dict(dtype=torch.int32)
    args = (torch.ones(1, 1, **i32), torch.tensor([2], **i32), torch.tensor([1], **i32))
    with pytest.raises(ValueError, match="GPU"):
        rnnt_loss_delay(x, *args, blank=4, delay_penalty=0.1)
    with pytest.raises(ValueError, match="GPU"):
        expected_emit_frames(x, *args, blank=4)
    with pytest.raises(ValueError, match="finite"):
        rnnt_loss_delay(x.to(DEV), *[a.to(DEV) for a in args], delay_penalty=float("nan"))


def test_expected_emit_frames_without_labels():
    """U = 1: costs, and frames of shape (N, 0)."""
    from warprnnt_pytorch.delay import expected_emit_frames
    x = torch.randn((2, 3, 1, 5), device=DEV)
    c, fr = expected_emit_frames(x, torch.zeros((2, 0), dtype=torch.int32, device=DEV), *dev(np.array([3, 2], np.int32),
                                                                                          np.array([0, 0], np.int32)))
    want = -torch.log_softmax(x, -1)[:, :, 0, 0]
    assert fr.shape == (2, 0) and torch.allclose(c, torch.stack((want[0].sum(), want[1, :2].sum())), rtol=1e-5)


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch), replayed twice on new logits."""
    from warprnnt_pytorch.delay import rnnt_loss_delay
    N, T, U, A, blank = 3, 8, 5, 33, 32
    rng = np.random.default_rng(11)
    tl, ll = np.array([8, 6, 4], np.int32), np.array([4, 0, 4], np.int32)
    labels = rng.integers(0, A - 1, size=(N, U - 1)).astype(np.int32)
    lab, ttl, tll = dev(labels, tl, ll)
    static_x = torch.zeros((N, T, U, A), device=DEV, requires_grad=True)
    m = _delay()
    m.lib()
    m.workspace_bytes(T, U, N, 0)

    def step():
        static_x.grad = None
        loss = rnnt_loss_delay(static_x, lab, ttl, tll, blank, 0.3, "sum", validate=False)
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
        loss = rnnt_loss_delay(static_x, lab, ttl, tll, blank, 0.3, "sum", validate=False)
        loss.backward()
    grad = static_x.grad
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    for seed in (1, 2):
        xn = np.random.default_rng(seed).standard_normal((N, T, U, A)).astype(np.float32)
        with torch.no_grad():
            static_x.copy_(torch.tensor(xn))
        graph.replay()
        torch.cuda.synchronize()
        rc, rg = R.delay_autograd(xn, labels, tl, ll, blank, PEN)
        assert abs(loss.item() - rc.sum()) < 1e-5 * abs(rc.sum())
        got = grad.double().cpu().numpy()
        assert not got[~mask].any()
        O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank)[mask], torch.float32, what="replay %d" % seed)


# ----------------------------------------------------------------------------- long utterances: the per-diagonal offsets
@pytest.mark.parametrize("U,A", [(301, 50), (33, 8)])
def test_long_utterance(U, A):
    """T = 1500, fp32, delay_penalty = 0.01: the bias reaches +-7.5 nats.  The block form's per-diagonal offsets (U = 301,
    the second sample short) and the wave form's per-chunk ones (U = 33, 191 re-centrings)."""
    N, T, blank = 2, 1500, A - 1
    pen = R.f32_penalty(0.01)
    tl, ll = np.array([T, 100], np.int32), np.array([U - 1, 30], np.int32)
    x, labels, tl, ll, mask = _problem("long", "f32", N, T, U, A, (tl, ll), scale=1.0, blank=blank)
    st, c, g, fr = call(x.to(DEV), labels, tl, ll, blank, pen, "one")
    assert st == 0
    rc, rg, re = _reference_all(x, labels, tl, ll, blank, pen)
    assert np.isfinite(rc).all()
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, what="long U = %d" % U)
    _check_emit("f32", fr, re, tl, ll, what="long U = %d" % U)


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_in_place_past_2_31_elements():
    """bf16 in place, N T U A > 2^31 elements: the last sample's rows lie past element 2^31.  The reference is taken over the
    few in-lattice rows only."""
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
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((N, T, U, A), generator=g, device=DEV, dtype=torch.bfloat16)
    small = torch.zeros((N, 4, 4, A), dtype=torch.float64)
    for b in range(N):
        small[b, :tl[b], :ll[b] + 1] = x[b, :tl[b], :ll[b] + 1].double().cpu()
    st, c, _, fr = call(x, labels, tl, ll, blank, PEN, "inplace")
    assert st == 0
    rc, rg = R.delay_autograd(small.numpy(), labels[:, :3], tl, ll, blank, PEN)
    assert np.isfinite(rc).all() and np.allclose(c, rc, rtol=1e-5, atol=1e-5), (c, rc)
    re = R.emit_frames_ref(small.numpy(), labels[:, :3], tl, ll, blank, PEN)
    assert not fr[:, 3:].any()
    _check_emit("bf16", fr[:, :3], re, tl, ll, what="past 2^31")
    inl = R.in_lattice_mask((N, 4, 4), tl, ll)
    for b in range(N):
        assert x[b, tl[b]:].count_nonzero().item() == 0
        assert x[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
        got = x[b, :4, :4].double().cpu().numpy()
        ref = rg[b]
        O.assert_grads(got[inl[b]], ref[inl[b]], np.maximum(np.abs(ref), np.abs(ref).sum(-1, keepdims=True))[inl[b]],
                       torch.bfloat16, what="sample %d" % b)
