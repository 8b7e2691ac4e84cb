"""-m gpu: the pruned RNN-T loss with k2's lattice types and delay_penalty (include/rnnt_pstream.h, libwarprnnt_pstream.so).

Every case of tests/pstream_forms.py runs through the one-call C-ABI entry under torch.profiler at delay_penalty = 0.3 with
gradients: exactly the kernels its release rules predict run, stage by stage.  Costs and gradients go through
gpu_support.check against the fp64 autograd reference of tests/pstream_ref.py (the bias written literally, no gauge): costs
at COST_TOL, gradients per element at oracle.grad_bound with mag = |ref| and, for the blank and label columns, the row's |ref|
sum; diagonals = T + U - 1 in the regular type, T in the modified one.  NaN in every row the header says is never read
(padding; the modified type: outside the band), gradient buffers that start as NaN.  The reference takes the penalty the
library sees: the value of the C-ABI's float.

Negative controls compare the modified type's result with the regular type's reference, and the result at 0.5 with the
reference at 0, and must fail.  Then the three identities of the header against the pruned, delay-penalized and monotonic
modules, the call forms, bit-identical reruns and workspaces, the invalid arguments, the non-finite cases, windows without a
path, bad starts, a label on the blank column, the autograd module, gradcheck, a HIP-graph capture, long utterances (where the
gauge is needed) and one bf16 tensor past 2^31 elements."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import pstream_forms as F
from tests import pstream_ref as R
from tests.gpu_support import (CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check,
                               dev, options, place, profiled, stages_seen)

pytestmark = pytest.mark.gpu
PEN = R.f32_penalty(0.3)


def _ps():
    from warprnnt_pytorch import pstream
    return pstream


def _problem(name, dtype, N, T, U, S, A, typ, tl, ll, s, rng=None, scale=2.0, blank=None):
    """Logits (N, T, S, A) with NaN in every row that is never read, labels over all of [0, A) but the blank, and the mask
    of the rows that are read."""
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = np.asarray(tl, np.int32), np.asarray(ll, np.int32)
    allowed = [c for c in range(A) if c != blank] or [0]
    labels = rng.choice(allowed, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]
    x = torch.tensor(rng.standard_normal((N, T, S, A)) * scale, dtype=torch.float32).to(TORCH[dtype])
    mask = R.read_mask((N, T, S), s, tl, ll, typ)
    x[torch.tensor(~mask)] = float("nan")
    return x, labels, mask


def _table_problem(name, case, seed=None):
    """(x, labels, s, tl, ll, mask) of a case-shaped dict: lengths and windows from the table's generators."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) if seed is None else seed)
    tl, ll = F.lengths(case, rng)
    s = F.ranges(case, tl, ll, rng)
    x, labels, mask = _problem(name, case["dtype"], case["N"], case["T"], case["U"], case["S"], case["A"], case["type"], tl, ll,
                               s, rng=rng, blank=case["blank"], scale=case.get("scale", 2.0))
    return x, labels, s, tl, ll, mask


def _shape(dtype, typ, N, T, U, S, A, blank, **kw):
    return dict(dtype=dtype, type=typ, N=N, T=T, U=U, S=S, A=A, blank=blank, **kw)


def call(x, labels, s, tl, ll, U, blank=0, typ=0, penalty=PEN, form="one", scale=None, grads=None, stream=None, prepare=1, ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host."""
    m = _ps()
    N, T, S, A = x.shape
    code = CODE[NAME[x.dtype]]
    pad = np.zeros((N, 1), np.int32)
    lab, ttl, tll, rg = dev(labels if labels.size else pad, tl, ll, np.asarray(s, np.int32))
    opt = options(T, U, blank, stream)
    lib = m.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    st, c, g = call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_rnnt_loss_pstream(x.data_ptr(), gp, rg.data_ptr(), S, typ, penalty, *lens, costs, ws,
                                                            opt, code),
        lambda costs, ws: lib.compute_rnnt_loss_pstream_fwd(x.data_ptr(), rg.data_ptr(), S, typ, penalty, *lens, costs, ws, opt,
                                                            code, prepare),
        lambda gp, sc, ws: lib.compute_rnnt_loss_pstream_bwd(x.data_ptr(), gp, sc, S, A, N, ws, opt, code),
        m.workspace_bytes(T, U, S, N, code), scale, grads, stream, ws)
    torch.cuda.synchronize()
    return st, c, g


def _clean(x):
    return torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()


def _reference(x, labels, s, tl, ll, blank=0, typ=0, penalty=PEN, weights=None):
    return R.pstream_autograd(_clean(x), labels, s, tl, ll, blank, typ, penalty, weights)


def _mag(ref, labels, s, ll, blank):
    """The size of the terms of every gradient element: |ref|, and for the blank and label columns the row's |ref| sum
    (they carry the subtracted posteriors).  The label of row (b, t, k) is that of state s[b, t] + k."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    mag[..., blank] = np.maximum(mag[..., blank], rs)
    N, T, S, _ = ref.shape
    u = np.asarray(s)[:, :T, None] + np.arange(S)[None, None, :]
    for b, t, k in zip(*np.nonzero((u >= 0) & (u < np.asarray(ll)[:, None, None]))):
        lab = int(labels[b, u[b, t, k]])
        mag[b, t, k, lab] = max(mag[b, t, k, lab], rs[b, t, k])
    return mag


def _check(dtype, got_c, got_g, ref_c, ref_g, mask, labels, s, ll, blank, typ, U, scale=None, what=""):
    T = mask.shape[1]
    check(dtype, got_c, got_g, ref_c, ref_g, mask,
          lambda ref, b: _mag(ref, labels[b:b + 1], np.asarray(s)[b:b + 1], ll[b:b + 1], blank), scale, what,
          diagonals=T if typ else T + U - 1)


# ----------------------------------------------------------------------------- every form of tests/pstream_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_pstream_form(name):
    case = F.CASES[name]
    cus = G.cus()
    dtype, blank, typ, U = case["dtype"], case["blank"], case["type"], case["U"]
    x, labels, s, tl, ll, mask = _table_problem(name, case)
    off = case.get("off", 0)
    xv = place(x.to(DEV), off, x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    (st, c, g), names = profiled(lambda: call(xv, labels, s, tl, ll, U, blank, typ, PEN, "one", grads=gv))
    if st == 0 and not any(F.stage_of(n) for n in names):    # (a profiler session now and then records no device event of
        print(name, "no kernel of the library recorded:", names)    # the call at all: one more session, judged as the first
        gv.fill_(float("nan"))                                    # would have been)
        (st, c, g), names = profiled(lambda: call(xv, labels, s, tl, ll, U, blank, typ, PEN, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, cus))
    rc, rg = _reference(x, labels, s, tl, ll, blank, typ)
    assert np.isfinite(rc).all()
    _check(dtype, c, g, rc, rg, mask, labels, s, ll, blank, typ, U, what=name)


def test_every_pstream_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_negative_controls(dtype):
    """The modified type's result against the regular type's reference, and the result at delay_penalty = 0.5 against the
    reference at 0, must fail for costs and for gradients: the checks cannot pass on another lattice or on the plain loss.
    Every sample has L_b >= 1 and T_b >= L_b + 2; the windows are whole (S = U), so both types read what the other reads
    inside the band."""
    N, T, U, A, blank = 4, 9, 5, 12, 11
    S = U
    tl, ll = np.array([9, 6, 7, 5], np.int32), np.array([4, 2, 1, 3], np.int32)
    s = np.zeros((N, T), np.int32)
    x, labels, mask1 = _problem("neg_" + dtype, dtype, N, T, U, S, A, 0, tl, ll, s, blank=blank)
    mask0 = R.read_mask((N, T, S), s, tl, ll, 0)
    mask1 = R.read_mask((N, T, S), s, tl, ll, 1)
    xd = x.to(DEV)
    refs = {(typ, p): _reference(x, labels, s, tl, ll, blank, typ, p) for typ in (0, 1) for p in (0.0, 0.5)}
    got = {}
    for typ, mask in ((0, mask0), (1, mask1)):
        st, c, g = call(xd, labels, s, tl, ll, U, blank, typ, 0.5, "one")
        assert st == 0
        got[typ] = (c, g)
        _check(dtype, c, g, *refs[typ, 0.5], mask, labels, s, ll, blank, typ, U, what="type %d" % typ)
    # on the CPU: the references differ
    for a, b in (((1, 0.5), (0, 0.5)), ((0, 0.5), (0, 0.0)), ((1, 0.5), (1, 0.0))):
        assert (np.abs(refs[a][0] - refs[b][0]) >= 100 * COST_TOL[dtype]).all(), (a, b, refs[a][0], refs[b][0])
        assert np.abs(refs[a][1] - refs[b][1]).max() >= 1e-2, (a, b)
    c1, g1 = got[1]
    c0, g0 = got[0]
    for what, c, g, (rc, rg), mask, typ in (("type 1 against type 0", c1, g1, refs[0, 0.5], mask1, 1),
                                             ("0.5 against 0, regular", c0, g0, refs[0, 0.0], mask0, 0),
                                             ("0.5 against 0, modified", c1, g1, refs[1, 0.0], mask1, 1)):
        with pytest.raises(AssertionError):
            _check(dtype, c, None, rc, rg, mask, labels, s, ll, blank, typ, U, what=what + ": costs")
        with pytest.raises(AssertionError):
            _check(dtype, rc, g, rc, rg, mask, labels, s, ll, blank, typ, U, what=what + ": gradients")


# ----------------------------------------------------------------------------- the identities of the header
def _identity_inputs(typ, full):
    N, T, U, A, blank = 4, 12, 5, 37, 9
    S = U if full else 3
    rng = np.random.default_rng(17 + typ)
    tl, ll = np.array([12, 1, 7, 9], np.int32), np.array([4, 1, 0, 3], np.int32)
    labels = rng.choice([c for c in range(A) if c != blank], size=(N, U - 1)).astype(np.int32)
    case = dict(N=N, T=T, U=U, S=S, type=typ)
    s = np.zeros((N, T), np.int32) if full else F.ranges(case, tl, ll, rng)
    x = torch.tensor(rng.standard_normal((N, T, S, A)) * 2, dtype=torch.float64, device=DEV)
    return x, labels, s, tl, ll, blank, U


def _both(x, mine, theirs):
    xa = x.clone().requires_grad_()
    la = mine(xa)
    la.sum().backward()
    xb = x.clone().requires_grad_()
    lb = theirs(xb)
    lb.sum().backward()
    assert torch.isfinite(la).all() and torch.allclose(la, lb, rtol=1e-9, atol=0), (la, lb)
    return xa.grad.cpu().numpy(), xb.grad.cpu().numpy()


def test_regular_without_penalty_is_the_pruned_loss():
    from warprnnt_pytorch.pruned import rnnt_loss_pruned
    x, labels, s, tl, ll, blank, U = _identity_inputs(0, full=False)
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    ga, gb = _both(x, lambda z: _ps().rnnt_loss_pruned_stream(z, lab, ttl, tll, rg, blank, "regular", 0.0, "none", False),
                   lambda z: rnnt_loss_pruned(z, lab, ttl, tll, rg, blank, "none", False))
    mask = R.in_lattice_mask(x.shape, s, tl, ll)
    assert not ga[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, s, ll, blank)[mask], torch.float64, what="pruned")


def test_regular_with_full_windows_is_the_delay_penalized_loss():
    from warprnnt_pytorch.delay import rnnt_loss_delay
    x, labels, s, tl, ll, blank, U = _identity_inputs(0, full=True)
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    ga, gb = _both(x, lambda z: _ps().rnnt_loss_pruned_stream(z, lab, ttl, tll, rg, blank, "regular", 0.3, "none", False),
                   lambda z: rnnt_loss_delay(z, lab, ttl, tll, blank, 0.3, "none", False))
    mask = R.in_lattice_mask(x.shape, s, tl, ll)
    assert not ga[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, s, ll, blank)[mask], torch.float64, what="delay")


def test_modified_with_full_windows_is_the_monotonic_loss():
    from warprnnt_pytorch.mono import rnnt_loss_mono
    x, labels, s, tl, ll, blank, U = _identity_inputs(1, full=True)
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    ga, gb = _both(x, lambda z: _ps().rnnt_loss_pruned_stream(z, lab, ttl, tll, rg, blank, "modified", 0.0, "none", False),
                   lambda z: rnnt_loss_mono(z, lab, ttl, tll, blank, "none", False))
    mask = R.read_mask(x.shape, s, tl, ll, 1)
    assert not ga[~mask].any() and not gb[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, s, ll, blank)[mask], torch.float64, what="mono")


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("dtype,U,typ", [("f32", 9, 0), ("bf16", 9, 1), ("f32", 66, 1), ("f64", 70, 0)])
def test_call_forms_agree(dtype, U, typ):
    case = _shape(dtype, typ, 5, 11 if U < 60 else 72, U, 4, 130, 129)
    N, T, S, blank = case["N"], case["T"], case["S"], case["blank"]
    x, labels, s, tl, ll, mask = _table_problem("forms_" + dtype, case, seed=U)
    xd = x.to(DEV)
    a = (labels, s, tl, ll, U, blank, typ, PEN)
    st, c1, g1 = call(xd, *a, "one")
    assert st == 0
    rc, rg = _reference(x, labels, s, tl, ll, blank, typ)
    _check(dtype, c1, g1, rc, rg, mask, labels, s, ll, blank, typ, U, what="one call")
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    st, c2, g2 = call(xd, *a, "two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    rcw, rgw = _reference(x, labels, s, tl, ll, blank, typ, weights=scale)
    _check(dtype, c2, g2, rcw, rgw, mask, labels, s, ll, blank, typ, U, what="two-phase")
    st, c2b, g2b = call(xd, *a, "two", scale=np.ones(N))
    assert st == 0 and np.array_equal(c1, c2b) and np.array_equal(g2b, g1)            # bit for bit at scale 1
    xi = xd.clone()
    st, c3, g3 = call(xi, *a, "inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1)
    st, c4, _ = call(xd, *a, "score")
    assert st == 0 and np.array_equal(c1, c4)
    st, c5, g5 = call(xd, *a, "host", grads=torch.full_like(xd, float("nan")))
    assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5) and np.array_equal(g5, g1)
    # a second run: identical bits
    st, c6, g6 = call(xd, *a, "one")
    assert st == 0 and np.array_equal(c1, c6) and np.array_equal(g1, g6)


@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("U", [6, 70])
def test_workspace_contents_do_not_matter(U, typ):
    """A workspace full of 0xFF bytes (NaN as values, -1 as flags) gives the bits a zeroed one gives: nothing an earlier call
    left reaches arithmetic -- the cells no row covers are written by the preparation kernel."""
    m = _ps()
    case = _shape("f32", typ, 5, 13 if U < 60 else 72, U, 3, 19, 3)
    N, T, S, A, blank = case["N"], case["T"], case["S"], case["A"], case["blank"]
    x, labels, s, tl, ll, mask = _table_problem("ws", case, seed=U + typ)
    xd = x.to(DEV)
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    out = []
    for fill in (0, 255):
        ws = torch.full((m.workspace_bytes(T, U, S, N, 0),), fill, dtype=torch.uint8, device=DEV)
        costs = torch.full((N,), float("nan"), device=DEV)
        g = torch.full_like(xd, float("nan"))
        st = m.lib().compute_rnnt_loss_pstream(xd.data_ptr(), g.data_ptr(), rg.data_ptr(), S, typ, PEN, lab.data_ptr(),
                                               tll.data_ptr(), ttl.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(),
                                               options(T, U, blank), 0)
        torch.cuda.synchronize()
        assert st == 0
        out.append((costs.cpu().numpy(), g.cpu().numpy()))
    assert np.isfinite(out[0][0]).all()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    rc, rgr = _reference(x, labels, s, tl, ll, blank, typ)
    _check("f32", out[1][0], out[1][1].astype(np.float64), rc, rgr, mask, labels, s, ll, blank, typ, U, what="0xFF workspace")


def test_invalid_arguments():
    m = _ps()
    N, T, U, S, A, blank = 2, 4, 3, 2, 7, 0
    tl, ll = np.array([4, 3], np.int32), np.array([2, 1], np.int32)
    s = np.array([[0, 0, 1, 1], [0, 0, 0, 0]], np.int32)
    x, labels, _ = _problem("inv", "f32", N, T, U, S, A, 0, tl, ll, s, blank=blank)
    xd = torch.nan_to_num(x.to(DEV))
    for typ in (0, 1):
        st, c, _ = call(xd, labels, s, tl, ll, U, blank, typ, PEN, "one")
        assert st == 0 and np.isfinite(c).all(), (typ, c)
    # a lattice type outside {0, 1}; a penalty that is not finite (negative ones are accepted)
    for bad in (-1, 2, 7):
        for form in ("one", "score", "host"):
            assert call(xd, labels, s, tl, ll, U, blank, bad, PEN, form)[0] == 2, (bad, form)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for form in ("one", "score", "host"):
            assert call(xd, labels, s, tl, ll, U, blank, 1, bad, form)[0] == 2, (bad, form)
    st, c, _ = call(xd, labels, s, tl, ll, U, blank, 0, -3.0, "one")
    assert st == 0 and np.isfinite(c).all()
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed, the
    # gradients of the bad one are zero
    assert call(xd, labels, s, np.array([T + 1, 3], np.int32), ll, U, blank, 0, PEN, "host")[0] == 2
    assert call(xd, labels, s, np.array([0, 3], np.int32), ll, U, blank, 1, PEN, "host")[0] == 2
    for bad_ll in (U, -1):
        st, c, g = call(xd, labels, s, tl, np.array([bad_ll, 1], np.int32), U, blank, 0, PEN, "one")
        assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
    for b in (A, -1):
        for form in ("one", "score"):
            assert call(xd, labels, s, tl, ll, U, b, 0, PEN, form)[0] == 2
    lib = m.lib()
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    costs = torch.zeros(N, device=DEV)
    ptrs = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr())
    one = lambda **kw: lib.compute_rnnt_loss_pstream(                                                        # noqa: E731
        kw.get("acts", xd.data_ptr()), kw.get("grads"), kw.get("ranges", rg.data_ptr()), kw.get("S", S), kw.get("typ", 0), PEN,
        *ptrs, kw.get("A", A), kw.get("N", N), costs.data_ptr(), kw.get("ws", ws.data_ptr()),
        kw.get("opt", options(T, U, blank)), kw.get("code", 0))
    assert one() == 0
    # the window size; maxU past the limit, maxT maxU >= 2^25, 2^32 cells and A past 2^23: refused before anything is touched
    for bad in (0, -1, U + 1):
        assert one(S=bad) == 2, bad
    assert one(opt=options(1, 4097, blank), S=1) == 2
    assert one(opt=options(1 << 13, 4096, blank)) == 2 and one(opt=options(1 << 12, 16, blank), N=1 << 16) == 2
    assert one(A=(1 << 23) + 1) == 2
    # dtype codes, the workspace query, NULL pointers, the CPU location
    n = C.c_size_t(0)
    q = lib.get_workspace_size_pstream
    assert q(4, 3, 2, 1, 4, C.byref(n)) == 2 and q(4, 3, 2, 1, -1, C.byref(n)) == 2 and q(0, 3, 2, 1, 0, C.byref(n)) == 2
    assert q(4, 3, 0, 1, 0, C.byref(n)) == 2 and q(4, 3, 4, 1, 0, C.byref(n)) == 2 and q(4, 3, 2, 1, 0, None) == 2
    assert q(4, 3, 2, 1, 0, C.byref(n)) == 0 and n.value > 0
    for code in (4, -1):
        assert one(code=code) == 2, code
    assert one(acts=None) == 2 and one(ws=None) == 2 and one(ranges=None) == 2
    assert lib.compute_rnnt_loss_pstream_bwd(xd.data_ptr(), None, None, S, A, N, ws.data_ptr(), options(T, U, blank), 0) == 2
    cpu = options(T, U, blank)
    cpu.loc = 0
    assert one(opt=cpu) == 2
    torch.cuda.synchronize()
    # gradients that overlap the activations without being them
    buf = torch.zeros(2 * xd.numel(), device=DEV)
    a = buf[:xd.numel()].view(xd.shape).copy_(xd)
    assert call(a, labels, s, tl, ll, U, blank, 0, PEN, "one", grads=buf[4:4 + xd.numel()].view(xd.shape))[0] == 2


@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_non_finite_inputs(dtype, typ):
    """NaN, +inf or an all -inf row that is read: that sample only -- NaN cost, NaN gradients on its in-lattice rows.  A
    -inf blank or label logit is a limit: finite cost while a path is left, +inf (and the same NaNs) when none is.  A NaN in
    a row that is never read changes nothing (every such row of the problem holds one)."""
    N, T, U, S, A, blank = 8, 6, 4, 3, 11, 6
    tl, ll = np.full(N, 5, np.int32), np.full(N, 2, np.int32)
    tl[0] = 6
    ll[6] = 3
    s = np.tile(np.array([0, 0, 0, 1, 1, 1], np.int32), (N, 1))
    s[ll == 2, 3:] = 0                                            # (L_b = 2: the three states fit one window)
    x, labels, mask = _problem("nf_%s_%d" % (dtype, typ), dtype, N, T, U, S, A, typ, tl, ll, s, blank=blank)
    inl = R.in_lattice_mask((N, T, S), s, tl, ll)
    inf = float("inf")
    x[1, 1, 0, 3] = float("nan")                                 # a NaN logit
    x[2, 2, 1, blank] = float("nan")                             # a NaN blank logit
    x[3, 1, 1, 8] = inf                                          # a +inf logit
    x[4, 3, 2, :] = -inf                                         # an all -inf row
    x[5, 1, 1, blank] = -inf                                     # no blank out of one cell: paths around it remain
    x[5, 0, 0, int(labels[5, 0])] = -inf                         # no label out of (0, 0): label 0 is emitted later
    x[6, 4, 2, blank] = -inf                                     # the last blank out of (4, 3) closed
    if typ == 1:
        x[6, 4, 1, int(labels[6, 2])] = -inf                     # ... and the label edge into the terminal node: no path
    x[7, :, 1, int(labels[7, 1])] = -inf                         # label 1 can never be emitted: no path
    st, c, g = call(x.to(DEV), labels, s, tl, ll, U, blank, typ, PEN, "one")
    assert st == 0
    for b in (1, 2, 3, 4):
        assert np.isnan(c[b]) and np.isnan(g[b][inl[b]]).all(), (b, c)
    for b in (6, 7):
        assert np.isposinf(c[b]) and np.isnan(g[b][inl[b]]).all(), (b, c)
    assert not g[~inl].any()
    keep = [0, 5]
    # the reference takes the limit at a logit of -200: autograd through -inf is NaN, and e^-200 is far below every bound
    xr = x[keep].float()
    xr[torch.tensor(~mask[keep])] = 0.0
    xr = torch.nan_to_num(xr, nan=0.0).clamp(min=-200.0).to(x.dtype)
    rc, rg = _reference(xr, labels[keep], s[keep], tl[keep], ll[keep], blank, typ)
    assert np.isfinite(rc).all()
    _check(dtype, c[keep], g[keep], rc, rg, mask[keep], labels[keep], s[keep], ll[keep], blank, typ, U, what="limits")


@pytest.mark.parametrize("U", [6, 70])
@pytest.mark.parametrize("typ", [0, 1])
def test_windows_without_a_path(typ, U):
    """Separating windows (sample 1), and in the modified type T_b < L_b (sample 2): +inf cost and NaN gradients on the
    in-lattice rows; samples 0 and 3 are unaffected."""
    N, T, S, A, blank = 4, 8, 2, 7, 0
    tl, ll = np.array([8, 8, 3 if typ else 8, 6], np.int32), np.array([5, 5, 5, 2], np.int32)
    rng = np.random.default_rng(U + typ)
    case = dict(N=N, T=T, U=U, S=S, type=typ)
    s = np.stack([R.windows(rng, int(tl[b]), int(ll[b]), S, typ, T) if R.max_labels(int(tl[b]), S, typ) >= ll[b]
                  else np.zeros(T, np.int32) for b in range(N)])
    s[1] = [0, 0, 0, 3, 3, 4, 4, 4]                               # states {0, 1} then {3, 4}: no edge crosses
    if typ == 0:
        s[2] = [0, 0, 1, 1, 1, 1, 4, 4]                           # (regular: a second separating pattern, {1, 2} then {4, 5})
    for b in (1, 2):
        assert not R.has_path(s[b], int(tl[b]), int(ll[b]), S, typ)
    x, labels, mask = _problem("nopath", "f32", N, T, U, S, A, typ, tl, ll, s, blank=blank)
    inl = R.in_lattice_mask((N, T, S), s, tl, ll)
    st, c, g = call(x.to(DEV), labels, s, tl, ll, U, blank, typ, PEN, "one")
    assert st == 0
    for b in (1, 2):
        assert np.isposinf(c[b]) and np.isnan(g[b][inl[b]]).all() and not g[b][~inl[b]].any(), (b, c)
    keep = [0, 3]
    rc, rg = _reference(x[keep], labels[keep], s[keep], tl[keep], ll[keep], blank, typ)
    assert np.isfinite(rc).all()
    _check("f32", c[keep], g[keep], rc, rg, mask[keep], labels[keep], s[keep], ll[keep], blank, typ, U, what="others")
    # host costs: +inf is a cost, not a refusal
    st, ch, _ = call(x.to(DEV), labels, s, tl, ll, U, blank, typ, PEN, "host", grads=torch.full_like(x, float("nan")).to(DEV))
    assert st == 0 and np.array_equal(np.isposinf(ch), np.isposinf(c))


@pytest.mark.parametrize("typ", [0, 1])
def test_bad_starts(typ):
    """A start outside [0, L_b] in a frame t < T_b: the cost marker, zero gradients, status 2 with host costs; the other
    samples are computed.  A start outside it in a frame past T_b is never looked at."""
    N, T, U, S, A, blank = 4, 6, 4, 2, 9, 8
    tl, ll = np.array([6, 5, 6, 4], np.int32), np.array([3, 2, 3, 1], np.int32)
    rng = np.random.default_rng(3 + typ)
    case = dict(N=N, T=T, U=U, S=S, type=typ)
    s = F.ranges(case, tl, ll, rng)
    good = s.copy()
    s[1, 2] = 3                                                   # L_1 = 2
    s[2, 0] = -1
    s[3, 5] = 77                                                  # T_3 = 4: padding
    x, labels, _ = _problem("bad", "f32", N, T, U, S, A, typ, tl, ll, good, blank=blank)
    x = torch.nan_to_num(x)
    st, c, g = call(x.to(DEV), labels, s, tl, ll, U, blank, typ, PEN, "one")
    assert st == 0
    assert np.isnan(c[1]) and np.isnan(c[2]) and not g[1].any() and not g[2].any()
    keep = [0, 3]
    mask = R.read_mask((N, T, S), good, tl, ll, typ)
    rc, rg = _reference(x[keep], labels[keep], good[keep], tl[keep], ll[keep], blank, typ)
    _check("f32", c[keep], g[keep], rc, rg, mask[keep], labels[keep], good[keep], ll[keep], blank, typ, U, what="good samples")
    st, _, gh = call(x.to(DEV), labels, s, tl, ll, U, blank, typ, PEN, "host", grads=torch.full_like(x, float("nan")).to(DEV))
    assert st == 2 and not gh[1].any() and not gh[2].any()
    st, ch, _ = call(x.to(DEV), labels, good, tl, ll, U, blank, typ, PEN, "host", grads=torch.full_like(x, float("nan")).to(DEV))
    assert st == 0 and np.isfinite(ch).all()


@pytest.mark.parametrize("typ", [0, 1])
def test_label_equal_to_the_blank(typ):
    """Legal: the column carries both edges' posteriors."""
    case = _shape("f32", typ, 3, 6, 4, 3, 9, 4)
    rng = np.random.default_rng(typ)
    tl, ll = np.array([6, 5, 6], np.int32), np.array([3, 2, 1], np.int32)
    s = F.ranges(case, tl, ll, rng)
    x, labels, mask = _problem("lab", "f32", 3, 6, 4, 3, 9, typ, tl, ll, s, blank=4)
    labels[0, 1] = 4
    labels[1, 0] = 4
    labels[1, 1] = 4
    labels[2, 2] = 4                   # behind L_2 = 1: never looked at
    st, c, g = call(x.to(DEV), labels, s, tl, ll, 4, 4, typ, PEN, "one")
    assert st == 0
    rc, rg = _reference(x, labels, s, tl, ll, 4, typ)
    assert np.isfinite(rc).all()
    _check("f32", c, g, rc, rg, mask, labels, s, ll, 4, typ, 4, what="label on the blank")


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("typ", ["regular", "modified"])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_reductions(reduction, typ):
    N, T, U, S, A, blank = 3, 6, 4, 2, 11, 10
    code = _ps().type_code(typ)
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 3], np.int32)
    s = F.ranges(dict(N=N, T=T, U=U, S=S, type=code), tl, ll, np.random.default_rng(2))
    x, labels, mask = _problem("ag", "f32", N, T, U, S, A, code, tl, ll, s, blank=blank)
    x = torch.nan_to_num(x)
    xd = x.to(DEV).requires_grad_()
    loss = _ps().PrunedStreamingRNNTLoss(blank=blank, rnnt_type=typ, delay_penalty=0.3, reduction=reduction)(
        xd, *dev(labels, tl, ll, s))
    go = torch.tensor([0.7, -1.3, 2.0][:loss.numel()], device=DEV).view(loss.shape)
    (loss * go).sum().backward()
    w = go.detach().cpu().numpy().reshape(-1)
    w = np.broadcast_to(w, (N,)) / (N if reduction == "mean" else 1)
    rc, rg = _reference(x, labels, s, tl, ll, blank, code, weights=w)
    want = {"none": rc, "sum": rc.sum(keepdims=True), "mean": rc.mean(keepdims=True)}[reduction]
    assert np.allclose(loss.detach().cpu().numpy(), want, rtol=1e-5)
    got = xd.grad.double().cpu().numpy()
    assert not got[~mask].any()
    O.assert_grads(got[mask], rg[mask], _mag(rg, labels, s, ll, blank)[mask], torch.float32)


@pytest.mark.parametrize("typ", ["regular", "modified"])
def test_gradcheck_fp64(typ):
    N, T, U, S, A, blank = 2, 4, 3, 2, 6, 2
    rng = np.random.default_rng(2)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    tl, ll = np.array([4, 3], np.int32), np.array([2, 1], np.int32)
    s = F.ranges(dict(N=N, T=T, U=U, S=S, type=_ps().type_code(typ)), tl, ll, rng)
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    x = torch.tensor(rng.standard_normal((N, T, S, A)), dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda z: _ps().rnnt_loss_pruned_stream(z, lab, ttl, tll, rg, blank, typ, 0.3, "none"), (x,),
                                    eps=1e-6, atol=1e-6, nondet_tol=1e-12)


def test_python_refusals_on_the_device():
    m = _ps()
    N, T, U, S, A = 2, 3, 5, 2, 5
    x = torch.zeros((N, T, S, A), device=DEV)
    lab = torch.ones((N, U - 1), dtype=torch.int32, device=DEV)
    ttl, tll = dev(np.array([3, 2], np.int32), np.array([4, 3], np.int32))
    rg = torch.zeros((N, T), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="sample 0 has T_b = 3 < L_b = 4"):
        m.rnnt_loss_pruned_stream(x, lab, ttl, tll, rg, rnnt_type="modified")
    loss = m.rnnt_loss_pruned_stream(x, lab, ttl, tll, rg, rnnt_type="modified", reduction="none", validate=False)
    assert torch.isposinf(loss).all()
    for bad in (rg.long(), rg[:, :2].contiguous(), rg.cpu()):
        with pytest.raises((ValueError, TypeError)):
            m.rnnt_loss_pruned_stream(x, lab, ttl, tll, bad)
    with pytest.raises(ValueError, match="window size"):
        m.rnnt_loss_pruned_stream(torch.zeros((N, T, U + 1, A), device=DEV), lab, ttl, tll, rg)
    with pytest.raises(ValueError, match="'regular' or 'modified'"):
        m.rnnt_loss_pruned_stream(x, lab, ttl, tll, rg, rnnt_type="constrained")
    with pytest.raises(ValueError, match="not a column"):
        m.rnnt_loss_pruned_stream(x, lab, ttl, tll, rg, blank=A)


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch) with validate=False, replayed twice on new logits."""
    m = _ps()
    N, T, U, S, A, blank = 3, 8, 5, 3, 33, 32
    rng = np.random.default_rng(11)
    tl, ll = np.array([8, 6, 5], np.int32), np.array([4, 0, 4], np.int32)
    labels = rng.integers(0, A - 1, size=(N, U - 1)).astype(np.int32)
    s = F.ranges(dict(N=N, T=T, U=U, S=S, type=1), tl, ll, rng)
    lab, ttl, tll, rg = dev(labels, tl, ll, s)
    static_x = torch.zeros((N, T, S, A), device=DEV, requires_grad=True)
    m.lib()
    m.workspace_bytes(T, U, S, N, 0)

    def step():
        static_x.grad = None
        loss = m.rnnt_loss_pruned_stream(static_x, lab, ttl, tll, rg, blank, "modified", 0.3, "sum", validate=False)
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
        loss = m.rnnt_loss_pruned_stream(static_x, lab, ttl, tll, rg, blank, "modified", 0.3, "sum", validate=False)
        loss.backward()
    grad = static_x.grad
    mask = R.read_mask((N, T, S), s, tl, ll, 1)
    for seed in (1, 2):
        xn = np.random.default_rng(seed).standard_normal((N, T, S, A)).astype(np.float32)
        with torch.no_grad():
            static_x.copy_(torch.tensor(xn))
        graph.replay()
        torch.cuda.synchronize()
        rc, rgr = R.pstream_autograd(xn, labels, s, tl, ll, blank, 1, PEN)
        assert abs(loss.item() - rc.sum()) < 1e-5 * abs(rc.sum())
        got = grad.double().cpu().numpy()
        assert not got[~mask].any()
        O.assert_grads(got[mask], rgr[mask], _mag(rgr, labels, s, ll, blank)[mask], torch.float32, what="replay %d" % seed)


# ----------------------------------------------------------------------------- long utterances: the gauge
@pytest.mark.parametrize("typ", [0, 1])
@pytest.mark.parametrize("U,S,A", [(301, 5, 50), (33, 4, 8)])
def test_long_utterance(U, S, A, typ):
    """T = 1500, fp32, delay_penalty = 0.01: a partial path's literal bias reaches hundreds of nats; the gauge of
    csrc/rnnt_pstream_kernels.h keeps the lattice values of a diagonal (a frame) together.  The block form's per-diagonal
    (per-frame) offsets at U = 301, the second sample short, and the wave form's per-chunk ones at U = 33."""
    N, T, blank = 2, 1500, A - 1
    pen = R.f32_penalty(0.01)
    case = _shape("f32", typ, N, T, U, S, A, blank, scale=1.0)
    tl, ll = np.array([T, 100], np.int32), np.array([U - 1, 30], np.int32)
    rng = np.random.default_rng(U + typ)
    s = F.ranges(case, tl, ll, rng)
    x, labels, mask = _problem("long", "f32", N, T, U, S, A, typ, tl, ll, s, rng=rng, scale=1.0, blank=blank)
    st, c, g = call(x.to(DEV), labels, s, tl, ll, U, blank, typ, pen, "one")
    assert st == 0
    rc, rg = _reference(x, labels, s, tl, ll, blank, typ, pen)
    assert np.isfinite(rc).all()
    _check("f32", c, g, rc, rg, mask, labels, s, ll, blank, typ, U, what="long U = %d type %d" % (U, typ))


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_in_place_past_2_31_elements():
    """bf16 in place, N T S A > 2^31 elements: the last sample's rows lie past element 2^31.  The modified type on whole
    windows (S = maxU, every start 0).  The reference is taken over the few in-lattice rows only."""
    N, T, U, A, blank = 5, 64, 65, 130001, 70000
    S = U
    E = N * T * S * A
    assert E > 2 ** 31 and 4 * T * S * A > 2 ** 31 - 3 * T * S * A
    need = 2 * E + (1 << 30)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        print("SKIPPED: %d bytes of device memory free, the tensor past 2^31 elements needs %d" % (free, need))
        pytest.skip("device memory is short")
    tl, ll = np.array([1, 2, 3, 2, 4], np.int32), np.array([0, 1, 2, 1, 3], np.int32)
    rng = np.random.default_rng(13)
    labels = rng.integers(4, 60000, size=(N, U - 1)).astype(np.int32)
    s = np.zeros((N, T), np.int32)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((N, T, S, A), generator=g, device=DEV, dtype=torch.bfloat16)
    small = torch.zeros((N, 4, 4, A), dtype=torch.float64)
    for b in range(N):
        small[b, :tl[b], :ll[b] + 1] = x[b, :tl[b], :ll[b] + 1].double().cpu()
    st, c, _ = call(x, labels, s, tl, ll, U, blank, 1, PEN, "inplace")
    assert st == 0
    rc, rg = R.pstream_autograd(small.numpy(), labels[:, :3], s[:, :4], tl, ll, blank, 1, PEN)
    assert np.isfinite(rc).all() and np.allclose(c, rc, rtol=1e-5, atol=1e-5), (c, rc)
    read = R.read_mask((N, 4, 4), s[:, :4], tl, ll, 1)
    for b in range(N):
        assert x[b, tl[b]:].count_nonzero().item() == 0
        assert x[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
        got = x[b, :4, :4].double().cpu().numpy()
        ref = rg[b]
        assert not got[~read[b]].any()
        O.assert_grads(got[read[b]], ref[read[b]], np.maximum(np.abs(ref), np.abs(ref).sum(-1, keepdims=True))[read[b]],
                       torch.bfloat16, what="sample %d" % b)
