"""-m gpu: the multi-blank transducer loss (include/rnnt_mblank.h, libwarprnnt_mblank.so).

Every case of tests/mblank_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules predict
run, stage by stage.  Costs and gradients go through gpu_support.check against the fp64 autograd reference of
tests/mblank_ref.py: costs at COST_TOL, gradients per element at oracle.grad_bound with mag = |ref| and, for the blank, big-blank
and label columns, the row's |ref| sum.  Ragged lengths (one sample with T_b = 1, one with L_b = 0), NaN in every padding row
(never read) and gradient buffers that start as NaN (padding must come back as exact zeros).  A negative control compares
against the plain RNN-T loss and must fail.  Then the K = 0 cross-check against RNNTLoss, the call forms, the invalid
arguments, the non-finite cases of the header, a label on a big-blank column, the autograd module, a HIP-graph capture, a long
utterance and one bf16 tensor past 2^31 elements."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import mblank_forms as F
from tests import mblank_ref as R
from tests.gpu_support import (CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check,
                               dev, options, place, profiled, ragged_lengths, stages_seen)

pytestmark = pytest.mark.gpu


def _mb():
    from warprnnt_pytorch import mblank
    return mblank


def _labels(rng, N, U, A, blank, cols):
    """Labels in [0, A) without the blank and the big-blank columns."""
    allowed = [c for c in range(A) if c != blank and c not in cols]
    return rng.choice(allowed, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]


def _problem(name, dtype, N, T, U, A, blank, cols, rng=None, lengths=None, scale=2.0):
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    if lengths is not None:
        tl, ll = np.asarray(lengths[0], np.int32), np.asarray(lengths[1], np.int32)
    else:
        tl, ll = ragged_lengths(N, T, U, rng)
    labels = _labels(rng, N, U, A, blank, cols)
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * scale, dtype=torch.float32).to(TORCH[dtype])
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    x[torch.tensor(~mask)] = float("nan")
    return x, labels, tl, ll, mask


def _arrays(cols, durs):
    return (C.c_int * max(len(cols), 1))(*cols), (C.c_int * max(len(durs), 1))(*durs)


def call(x, labels, tl, ll, cols, durs, blank=0, form="one", scale=None, grads=None, sigma=0.0, stream=None, K=None, ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host."""
    m = _mb()
    N, T, U, A = x.shape
    K = len(durs) if K is None else K
    code = CODE[NAME[x.dtype]]
    lab, ttl, tll = dev(labels if labels.size else np.zeros((N, 1), np.int32), tl, ll)
    carr, darr = _arrays(cols, durs)
    opt = options(T, U, blank, stream)
    lib = m.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    return call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_mblank_loss(x.data_ptr(), gp, carr, darr, K, sigma, *lens, costs, ws, opt, code),
        lambda costs, ws: lib.compute_mblank_loss_fwd(x.data_ptr(), carr, darr, K, sigma, *lens, costs, ws, opt, code, 1),
        lambda gp, sc, ws: lib.compute_mblank_loss_bwd(x.data_ptr(), gp, sc, carr, darr, K, A, N, ws, opt, code),
        m.workspace_bytes(T, U, N, min(max(K, 0), 8), code), scale, grads, stream, ws)


def _reference(x, labels, tl, ll, cols, durs, blank=0, sigma=0.0, weights=None):
    xr = torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()
    return R.mblank_autograd(xr, labels, tl, ll, cols, durs, blank, sigma, weights)


def _mag(ref, labels, ll, blank, cols):
    """The size of the terms of every gradient element: |ref|, and for the blank, big-blank and label columns the row's |ref|
    sum (they carry the subtracted posteriors)."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    for c in (blank,) + tuple(cols):
        mag[..., c] = np.maximum(mag[..., c], rs)
    N, T, U, _ = ref.shape
    for b in range(N):
        for u in range(min(U, int(ll[b]))):
            lab = int(labels[b, u])
            mag[b, :, u, lab] = np.maximum(mag[b, :, u, lab], rs[b, :, u])
    return mag


def _check(dtype, got_c, got_g, ref_c, ref_g, mask, labels, ll, blank, cols, scale=None, what=""):
    check(dtype, got_c, got_g, ref_c, ref_g, mask, lambda ref, b: _mag(ref, labels[b:b + 1], ll[b:b + 1], blank, cols), scale,
          what, diagonals=mask.shape[1] + labels.shape[1])


# ----------------------------------------------------------------------------- every form of tests/mblank_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_mblank_form(name):
    case = F.CASES[name]
    cus = G.cus()
    N, T, U, A, dtype = case["N"], case["T"], case["U"], case["A"], case["dtype"]
    blank, cols, durs = case["blank"], case["columns"], case["durations"]
    x, labels, tl, ll, mask = _problem(name, dtype, N, T, U, A, blank, cols, lengths=case.get("lengths"))
    off = case.get("off", 0)
    xv = place(x.to(DEV), off, x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, cols, durs, blank, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, cus))
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank)
    assert np.isfinite(rc).all()                     # (the standard blank always leaves a path)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, cols, what=name)


def test_every_mblank_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


def test_sigma_and_explicit_columns():
    N, T, U, A, blank, cols, durs = 4, 10, 6, 37, 20, (36, 0, 19), (2, 3, 7)
    x, labels, tl, ll, mask = _problem("sigma", "f32", N, T, U, A, blank, cols)
    st, c, g = call(x.to(DEV), labels, tl, ll, cols, durs, blank, "one", sigma=0.05)
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank, 0.05)
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, cols, what="sigma")


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_negative_control_plain_rnnt_is_refused(dtype):
    """The same comparison against the plain RNN-T loss, the big-blank columns left as ordinary unused columns, must fail:
    the check cannot pass on the wrong loss.  Every T_b >= 2, so that a big blank fits in every sample."""
    N, T, U, A, blank, cols, durs = 4, 9, 7, 12, 11, (10, 9), (2, 4)
    lengths = ((9, 5, 7, 3), (6, 2, 0, 1))
    x, labels, tl, ll, mask = _problem("neg_" + dtype, dtype, N, T, U, A, blank, cols, lengths=lengths)
    st, c, g = call(x.to(DEV), labels, tl, ll, cols, durs, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, cols, what="multi-blank")
    pc, pg = _reference(x, labels, tl, ll, (), (), blank)
    assert (np.abs(pc - rc) >= 100 * COST_TOL[dtype]).all(), (pc, rc)
    with pytest.raises(AssertionError):
        _check(dtype, c, None, pc, pg, mask, labels, ll, blank, cols, what="plain costs")
    with pytest.raises(AssertionError):
        _check(dtype, rc, g, rc, pg, mask, labels, ll, blank, cols, what="plain gradients")


def test_without_big_blanks_it_is_rnntloss():
    """K = 0, sigma = 0 against RNNTLoss on the same tensor, fp64, on the GPU."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.mblank import MultiBlankLoss
    N, T, U, A, blank = 4, 12, 8, 37, 9
    rng = np.random.default_rng(17)
    tl, ll = ragged_lengths(N, T, U, rng)
    tl[1] = 3
    labels = _labels(rng, N, U, A, blank, ())
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * 2, dtype=torch.float64, device=DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    xa = x.clone().requires_grad_()
    la = MultiBlankLoss((), blank=blank, reduction="none")(xa, lab, ttl, tll)
    la.sum().backward()
    xb = x.clone().requires_grad_()
    lb = RNNTLoss(blank=blank, reduction="none")(xb, lab, ttl, tll)
    lb.sum().backward()
    assert torch.allclose(la, lb, rtol=1e-9, atol=1e-9), (la, lb)
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    ga, gb = xa.grad.cpu().numpy(), xb.grad.cpu().numpy()
    assert not ga[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, ll, blank, ())[mask], torch.float64, what="cross-check")


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_call_forms_agree(dtype):
    N, T, U, A, blank, durs = 5, 7, 9, 130, 129, (2, 4, 8)
    cols = F.nemo_columns(blank, 3)
    x, labels, tl, ll, mask = _problem("forms_" + dtype, dtype, N, T, U, A, blank, cols)
    xd = x.to(DEV)
    st, c1, g1 = call(xd, labels, tl, ll, cols, durs, blank, "one")
    assert st == 0
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    st, c2, g2 = call(xd, labels, tl, ll, cols, durs, blank, "two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank, weights=scale)
    _check(dtype, c2, g2, rc, rg, mask, labels, ll, blank, cols, what="two-phase")
    g1s = g1 * scale[:, None, None, None]
    assert np.allclose(g2, g1s, rtol=1e-2 if dtype == "bf16" else 1e-6, atol=1e-6)
    xi = xd.clone()
    st, c3, g3 = call(xi, labels, tl, ll, cols, durs, blank, "inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1)
    st, c4, _ = call(xd, labels, tl, ll, cols, durs, blank, "score")
    assert st == 0 and np.array_equal(c1, c4)
    st, c5, g5 = call(xd, labels, tl, ll, cols, durs, blank, "host", grads=torch.full_like(xd, float("nan")))
    assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5) and np.array_equal(g5, g1)


def test_invalid_arguments():
    m = _mb()
    N, T, U, A, blank = 2, 4, 3, 7, 0
    x, labels, tl, ll, _ = _problem("inv", "f32", N, T, U, A, blank, (5, 6))
    xd = torch.nan_to_num(x.to(DEV))
    ok = ((5, 6), (2, 3))
    st, c, _ = call(xd, labels, tl, ll, *ok, blank, "one")
    assert st == 0 and np.isfinite(c).all()
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed
    st, c, _ = call(xd, labels, np.array([T + 1, T], np.int32), ll, *ok, blank, "host")
    assert st == 2
    st, c, g = call(xd, labels, np.array([T, T], np.int32), np.array([U, 1], np.int32), *ok, blank, "one")
    assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
    bad = {"K = 9": (tuple(range(1, 10)), tuple(range(2, 11))),
           "duration 1": ((5, 6), (1, 3)), "duration 65": ((5, 6), (2, 65)),
           "durations not increasing": ((5, 6), (3, 3)), "durations decreasing": ((5, 6), (4, 2)),
           "a column equal to the blank": ((5, blank), (2, 3)), "a duplicate column": ((5, 5), (2, 3)),
           "a column past A": ((5, A), (2, 3)), "a negative column": ((-1, 6), (2, 3))}
    for what, (cols, durs) in bad.items():
        for form in ("one", "score"):
            st, _, _ = call(xd, labels, tl, ll, cols, durs, blank, form)
            assert st == 2, (what, form)
    st, _, _ = call(xd, labels, tl, ll, (), (), blank, "one", K=-1)
    assert st == 2
    for b in (A, -1):
        st, _, _ = call(xd, labels, tl, ll, *ok, b, "one")
        assert st == 2
    # maxU past the limit, dtype codes, the workspace query, overlapping tensors
    xb = torch.zeros((1, 1, 4097, 3), device=DEV)
    st, _, _ = call(xb, np.zeros((1, 4096), np.int32), np.array([1], np.int32), np.array([0], np.int32), (), (), 0, "one")
    assert st == 2
    n = C.c_size_t(0)
    lib = m.lib()
    assert lib.get_workspace_size_mblank(4, 3, 1, 9, 0, C.byref(n)) == 2
    assert lib.get_workspace_size_mblank(4, 3, 1, -1, 0, C.byref(n)) == 2
    assert lib.get_workspace_size_mblank(4, 3, 1, 2, 4, C.byref(n)) == 2
    assert lib.get_workspace_size_mblank(4, 3, 1, 0, 0, C.byref(n)) == 0 and n.value > 0
    lab, ttl, tll = dev(labels, tl, ll)
    carr, darr = _arrays(*ok)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    costs = torch.zeros(N, device=DEV)
    for code in (4, -1):
        st = lib.compute_mblank_loss(xd.data_ptr(), None, carr, darr, 2, 0.0, lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(),
                                     A, N, costs.data_ptr(), ws.data_ptr(), options(T, U, blank), code)
        assert st == 2, code
    buf = torch.zeros(2 * xd.numel(), device=DEV)
    a = buf[:xd.numel()].view(xd.shape).copy_(xd)
    st, _, _ = call(a, labels, tl, ll, *ok, blank, "one", grads=buf[4:4 + xd.numel()].view(xd.shape))
    assert st == 2


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_non_finite_inputs(dtype):
    """NaN, +inf or an all -inf row inside the lattice: that sample only.  A -inf blank logit is a limit: finite cost while a
    path is left, +inf when none is."""
    N, T, U, A, blank, cols, durs = 8, 5, 3, 11, 6, (0, 10), (2, 4)
    rng = np.random.default_rng(5)
    tl, ll = np.full(N, 4, np.int32), np.full(N, 2, np.int32)
    tl[0] = 5
    tl[6] = 1                                                    # every big blank overshoots
    tl[7] = 3                                                    # duration 4 overshoots, duration 2 enters from (1, 2)
    x, labels, tl, ll, mask = _problem("nf_" + dtype, dtype, N, T, U, A, blank, cols, rng=rng, lengths=(tl, ll))
    inf = float("inf")
    x[1, 1, 0, 3] = float("nan")                                 # a NaN label logit
    x[2, 2, 1, cols[0]] = float("nan")                           # a NaN big-blank logit
    x[3, 0, 1, 8] = inf                                          # a +inf logit
    x[4, 3, 2, :] = -inf                                         # an all -inf row
    x[5, 1, 1, blank] = -inf                                     # no standard blank out of one cell: paths around it remain
    x[5, 2, 0, cols[0]] = -inf
    x[6, 0, 2, blank] = -inf                                     # the only cell that reaches the terminal node: no path
    x[7, 2, 2, blank] = -inf                                     # both ways into the terminal node closed: no path
    x[7, 1, 2, cols[0]] = -inf
    st, c, g = call(x.to(DEV), labels, tl, ll, cols, durs, blank, "one")
    assert st == 0
    for b in (1, 2, 3, 4):
        assert np.isnan(c[b]) and np.isnan(g[b][mask[b]]).all(), (b, c)
    for b in (6, 7):
        assert np.isposinf(c[b]) and np.isnan(g[b][mask[b]]).all(), (b, c)
    assert not g[~mask].any()
    keep = [0, 5]
    # the reference takes the limit at a logit of -200: autograd through -inf is NaN, and e^-200 is far below every bound
    xr = torch.nan_to_num(x[keep].float(), nan=0.0).clamp(min=-200.0).to(x.dtype)
    rc, rg = _reference(xr, labels[keep], tl[keep], ll[keep], cols, durs, blank)
    assert np.isfinite(rc).all()
    _check(dtype, c[keep], g[keep], rc, rg, mask[keep], labels[keep], ll[keep], blank, cols, what="limits")


def test_label_on_a_big_blank_column():
    """Legal at the C-ABI: the column carries both edges' posteriors.  The Python module refuses it."""
    N, T, U, A, blank, cols, durs = 3, 6, 4, 9, 4, (7, 2), (2, 3)
    rng = np.random.default_rng(21)
    tl, ll = np.array([6, 5, 6], np.int32), np.array([3, 2, 1], np.int32)
    x, labels, tl, ll, mask = _problem("lab", "f32", N, T, U, A, blank, cols, rng=rng, lengths=(tl, ll))
    labels[0, 1] = cols[0]
    labels[1, 0] = blank
    labels[1, 1] = cols[1]
    labels[2, 2] = cols[0]             # behind L_2 = 1: never looked at
    st, c, g = call(x.to(DEV), labels, tl, ll, cols, durs, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank)
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, cols, what="label on a big blank")
    from warprnnt_pytorch.mblank import rnnt_loss_mblank
    xd = torch.nan_to_num(x).to(DEV)
    with pytest.raises(ValueError, match="big-blank"):
        rnnt_loss_mblank(xd, *dev(labels, tl, ll), durs, blank=blank, big_blank_columns=cols, reduction="none")
    labels[0, 1], labels[1, 0], labels[1, 1] = 0, 0, 0
    out = rnnt_loss_mblank(xd, *dev(labels, tl, ll), durs, blank=blank, big_blank_columns=cols, reduction="none")
    assert torch.isfinite(out).all()


def test_closed_form_two_paths():
    """T = d, L = 0, K = 1: d standard blanks or one big blank."""
    A, blank, col = 5, 1, 3
    rng = np.random.default_rng(4)
    for d in (2, 5, 64):
        x = torch.tensor(rng.standard_normal((1, d, 1, A)), dtype=torch.float64)
        st, c, _ = call(x.to(DEV), np.zeros((1, 0), np.int32), np.array([d], np.int32), np.zeros(1, np.int32), (col,), (d,),
                        blank, "score")
        lp = torch.log_softmax(x[0, :, 0], -1).numpy()
        want = -np.logaddexp(lp[:, blank].sum(), lp[0, col])
        assert st == 0 and abs(c[0] - want) < 1e-9 * max(1.0, abs(want)), (d, c, want)


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_reductions(reduction):
    from warprnnt_pytorch.mblank import MultiBlankLoss
    N, T, U, A, blank, durs = 3, 6, 4, 11, 10, (2, 4)
    cols = F.nemo_columns(blank, 2)
    rng = np.random.default_rng(3)
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 1], np.int32)
    x, labels, tl, ll, mask = _problem("ag", "f32", N, T, U, A, blank, cols, rng=rng, lengths=(tl, ll))
    x = torch.nan_to_num(x)
    xd = x.to(DEV).requires_grad_()
    loss = MultiBlankLoss(durs, blank=blank, sigma=0.05, reduction=reduction)(xd, *dev(labels, tl, ll))
    go = torch.tensor([0.7, -1.3, 2.0][:loss.numel()], device=DEV).view(loss.shape)
    (loss * go).sum().backward()
    w = go.detach().cpu().numpy().reshape(-1)
    w = np.broadcast_to(w, (N,)) / (N if reduction == "mean" else 1)
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank, 0.05, weights=w)
    want = {"none": rc, "sum": rc.sum(keepdims=True), "mean": rc.mean(keepdims=True)}[reduction]
    assert np.allclose(loss.detach().cpu().numpy(), want, rtol=1e-5)
    got = xd.grad.double().cpu().numpy()
    assert not got[~mask].any()
    O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank, cols)[mask], torch.float32)


def test_gradcheck_fp64():
    from warprnnt_pytorch.mblank import rnnt_loss_mblank
    N, T, U, A, blank, cols, durs = 2, 4, 3, 6, 2, (5,), (2,)
    rng = np.random.default_rng(2)
    labels = _labels(rng, N, U, A, blank, cols)
    lab, ttl, tll = dev(labels, np.array([4, 3], np.int32), np.array([2, 1], np.int32))
    x = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda z: rnnt_loss_mblank(z, lab, ttl, tll, durs, blank, cols, 0.0, "none"), (x,),
                                    eps=1e-6, atol=1e-6, nondet_tol=1e-12)


def test_cpu_tensors_are_refused():
    from warprnnt_pytorch.mblank import rnnt_loss_mblank
    x = torch.zeros(1, 2, 2, 5)
    with pytest.raises(ValueError, match="GPU"):
        rnnt_loss_mblank(x, torch.ones(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                         torch.tensor([1], dtype=torch.int32), (2,), blank=4)


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch), replayed on new logits."""
    from warprnnt_pytorch.mblank import rnnt_loss_mblank
    N, T, U, A, blank, durs = 3, 8, 5, 33, 32, (2, 4, 8)
    cols = F.nemo_columns(blank, 3)
    rng = np.random.default_rng(11)
    tl, ll = np.array([8, 6, 4], np.int32), np.array([4, 0, 2], np.int32)
    labels = _labels(rng, N, U, A, blank, cols)
    lab, ttl, tll = dev(labels, tl, ll)
    static_x = torch.zeros((N, T, U, A), device=DEV, requires_grad=True)
    m = _mb()
    m.lib()
    m.workspace_bytes(T, U, N, 3, 0)

    def step():
        static_x.grad = None
        loss = rnnt_loss_mblank(static_x, lab, ttl, tll, durs, blank, None, 0.0, "sum", validate=False)
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
        loss = rnnt_loss_mblank(static_x, lab, ttl, tll, durs, blank, None, 0.0, "sum", validate=False)
        loss.backward()
    grad = static_x.grad
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    for seed in (1, 2):
        xn = np.random.default_rng(seed).standard_normal((N, T, U, A)).astype(np.float32)
        with torch.no_grad():
            static_x.copy_(torch.tensor(xn))
        graph.replay()
        torch.cuda.synchronize()
        rc, rg = R.mblank_autograd(xn, labels, tl, ll, cols, durs, blank)
        assert abs(loss.item() - rc.sum()) < 1e-5 * rc.sum()
        got = grad.double().cpu().numpy()
        assert not got[~mask].any()
        O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank, cols)[mask], torch.float32, what="replay %d" % seed)


# ----------------------------------------------------------------------------- a long utterance: the diagonal offsets
def test_long_utterance():
    """T = 1500, U = 301 (1800 anti-diagonals), fp32; the second sample is short, so that the fp64 reference (a Python loop
    over frames) takes about a second."""
    N, T, U, A, blank, durs = 2, 1500, 301, 50, 49, (2, 4, 8)
    cols = F.nemo_columns(blank, 3)
    rng = np.random.default_rng(7)
    lengths = (np.array([T, 100], np.int32), np.array([U - 1, 30], np.int32))
    x, labels, tl, ll, mask = _problem("long", "f32", N, T, U, A, blank, cols, rng=rng, lengths=lengths, scale=1.0)
    st, c, g = call(x.to(DEV), labels, tl, ll, cols, durs, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, cols, durs, blank)
    assert np.isfinite(rc).all()
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, cols, what="long")


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_in_place_past_2_31_elements():
    """bf16 in place, N T U A > 2^31 elements: the last sample's in-lattice rows lie past element 2^31.  The reference is
    taken over the few in-lattice rows only."""
    N, T, U, A, blank, durs = 5, 64, 65, 130001, 70000, (2, 3)
    cols = (130000, 3)
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
    st, c, _ = call(x, labels, tl, ll, cols, durs, blank, "inplace")
    assert st == 0
    rc, rg = R.mblank_autograd(small.numpy(), labels[:, :3], tl, ll, cols, durs, blank)
    assert np.allclose(c, rc, rtol=1e-5, atol=1e-5), (c, rc)
    for b in range(N):
        assert x[b, tl[b]:].count_nonzero().item() == 0
        assert x[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
        got = x[b, :tl[b], :ll[b] + 1].double().cpu().numpy()
        ref = rg[b, :tl[b], :ll[b] + 1]
        O.assert_grads(got, ref, np.maximum(np.abs(ref), np.abs(ref).sum(-1, keepdims=True)), torch.bfloat16,
                       what="sample %d" % b)
