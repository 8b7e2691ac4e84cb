"""-m gpu: the Hybrid Autoregressive Transducer loss (include/rnnt_hat.h, libwarprnnt_hat.so).

Every case of tests/hat_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules predict run,
stage by stage.  Costs are compared with the fp64 autograd reference of tests/hat_ref.py at rtol = atol = 1e-5 (1e-9 for fp64),
gradients per element at oracle.grad_bound with mag = |ref| and, for the blank and label columns, the row's |ref| sum.  Ragged
lengths (one sample with T_b = 1, one with L_b = 0), NaN in every padding row (never read) and gradient buffers that start as
NaN (padding must come back as exact zeros).  A negative control compares against the plain RNN-T loss and must fail.  Then
the call forms, the invalid arguments, the non-finite cases of the header, |z_blank| = 80, the cross-check against
RNNTLoss(hat_log_probs(z)), the autograd module, a HIP-graph capture, one bf16 tensor past 2^31 elements, and c3- / c4-shaped
problems."""
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import hat_forms as F
from tests import hat_ref as R
from tests.gpu_support import (CODE, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check, dev,
                               options, place, profiled, ragged_lengths, stages_seen)

pytestmark = pytest.mark.gpu


def _hat():
    from warprnnt_pytorch import hat
    return hat


def _labels(rng, N, U, A, blank):
    """Labels in [0, A) without the blank."""
    lab = rng.integers(0, A - 1, size=(N, U - 1)).astype(np.int32)
    return lab + (lab >= blank)


def _problem(name, dtype, N, T, U, A, blank, rng=None, lengths=None, scale=2.0):
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = lengths if lengths is not None else ragged_lengths(N, T, U, rng)
    labels = _labels(rng, N, U, A, blank)
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * scale, dtype=torch.float32).to(TORCH[dtype])
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    x[torch.tensor(~mask)] = float("nan")
    return x, labels, tl, ll, mask


def call(x, labels, tl, ll, blank=0, form="one", scale=None, grads=None, stream=None, ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host."""
    h = _hat()
    N, T, U, A = x.shape
    code = CODE[NAME[x.dtype]]
    lab, ttl, tll = dev(labels if labels.size else np.zeros((N, 1), np.int32), tl, ll)
    opt = options(T, U, blank, stream)
    lib = h.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    return call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_hat_loss(x.data_ptr(), gp, *lens, costs, ws, opt, code),
        lambda costs, ws: lib.compute_hat_loss_fwd(x.data_ptr(), *lens, costs, ws, opt, code, 1),
        lambda gp, sc, ws: lib.compute_hat_loss_bwd(x.data_ptr(), gp, sc, A, N, ws, opt, code),
        h.workspace_bytes(T, U, N, code), scale, grads, stream, ws)


def _reference(x, labels, tl, ll, blank=0, weights=None, plain=False):
    xr = torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()
    return R.hat_autograd(xr, labels, tl, ll, blank, weights, plain)


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


def _check(dtype, got_c, got_g, ref_c, ref_g, mask, labels, ll, blank=0, scale=None, what=""):
    """No sample of this loss is without a path while its logits are finite: a +inf reference cost is a fault."""
    check(dtype, got_c, got_g, ref_c, ref_g, mask, lambda ref, b: _mag(ref, labels[b:b + 1], ll[b:b + 1], blank), scale, what,
          infinite_ok=False, diagonals=mask.shape[1] + labels.shape[1])


# ----------------------------------------------------------------------------- every form of tests/hat_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_hat_form(name):
    case = F.CASES[name]
    cus = G.cus()
    N, T, U, A, blank, dtype = case["N"], case["T"], case["U"], case["A"], case["blank"], case["dtype"]
    x, labels, tl, ll, mask = _problem(name, dtype, N, T, U, A, blank)
    off = case.get("off", 0)
    xv = place(x.to(DEV), off, x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, blank, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, cus))
    rc, rg = _reference(x, labels, tl, ll, blank)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what=name)


def test_every_hat_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_negative_control_plain_rnnt_is_refused(dtype):
    """The same comparison against the loss with the blank column left inside the label softmax (plain RNN-T) must fail:
    the check cannot pass on the wrong loss."""
    N, T, U, A, blank = 4, 9, 7, 40, 13
    x, labels, tl, ll, mask = _problem("neg_" + dtype, dtype, N, T, U, A, blank)
    st, c, g = call(x.to(DEV), labels, tl, ll, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, blank)
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what="hat")
    pc, pg = _reference(x, labels, tl, ll, blank, plain=True)
    with pytest.raises(AssertionError):
        _check(dtype, c, None, pc, pg, mask, labels, ll, blank, what="plain costs")
    with pytest.raises(AssertionError):
        _check(dtype, rc, g, rc, pg, mask, labels, ll, blank, what="plain gradients")


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_call_forms_agree(dtype):
    N, T, U, A, blank = 5, 7, 9, 130, 77
    x, labels, tl, ll, mask = _problem("forms_" + dtype, dtype, N, T, U, A, blank)
    xd = x.to(DEV)
    st, c1, g1 = call(xd, labels, tl, ll, blank, "one")
    assert st == 0
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    st, c2, g2 = call(xd, labels, tl, ll, blank, "two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    rc, rg = _reference(x, labels, tl, ll, blank, weights=scale)
    _check(dtype, c2, g2, rc, rg, mask, labels, ll, blank, what="two-phase")
    g1s = g1 * scale[:, None, None, None]
    assert np.allclose(g2, g1s, rtol=1e-2 if dtype == "bf16" else 1e-6, atol=1e-6)
    xi = xd.clone()
    st, c3, g3 = call(xi, labels, tl, ll, blank, "inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1)
    st, c4, _ = call(xd, labels, tl, ll, blank, "score")
    assert st == 0 and np.array_equal(c1, c4)
    st, c5, g5 = call(xd, labels, tl, ll, blank, "host", grads=torch.full_like(xd, float("nan")))
    assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5) and np.array_equal(g5, g1)


def test_invalid_arguments():
    N, T, U, A = 2, 4, 3, 5
    x, labels, tl, ll, _ = _problem("inv", "f32", N, T, U, A, 0)
    xd = torch.nan_to_num(x.to(DEV))
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed
    st, c, _ = call(xd, labels, np.array([T + 1, T], np.int32), ll, 0, "host")
    assert st == 2
    st, c, g = call(xd, labels, np.array([T, T], np.int32), np.array([U, 1], np.int32), 0, "one")
    assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any()
    # blank outside the columns, a single column, maxU past the limit, a dtype code, overlapping tensors
    for blank in (A, -1):
        st, _, _ = call(xd, labels, tl, ll, blank, "one")
        assert st == 2
    st, _, _ = call(torch.zeros((1, 2, 1, 1), device=DEV), np.zeros((1, 0), np.int32), np.array([2], np.int32),
                    np.array([0], np.int32), 0, "one")
    assert st == 2
    h = _hat()
    import ctypes as C
    n = C.c_size_t(0)
    assert h.lib().get_workspace_size_hat(4, 1025, 1, 0, C.byref(n)) == 2
    assert h.lib().get_workspace_size_hat(4, 3, 1, 4, C.byref(n)) == 2
    assert h.lib().get_workspace_size_hat(4, 3, 1, 0, C.byref(n)) == 0 and n.value > 0
    buf = torch.zeros(2 * xd.numel(), device=DEV)
    a = buf[:xd.numel()].view(xd.shape).copy_(xd)
    st, _, _ = call(a, labels, tl, ll, 0, "one", grads=buf[4:4 + xd.numel()].view(xd.shape))
    assert st == 2


def test_label_equal_to_blank_poisons_its_sample_only():
    N, T, U, A, blank = 3, 5, 4, 9, 4
    rng = np.random.default_rng(21)
    tl, ll = np.array([5, 4, 5], np.int32), np.array([3, 2, 1], np.int32)
    x, labels, tl, ll, mask = _problem("lab", "f32", N, T, U, A, blank, rng=rng, lengths=(tl, ll))
    labels[1, 1] = blank               # inside L_1 = 2: poisons sample 1
    labels[2, 2] = blank               # behind L_2 = 1: never looked at
    st, c, g = call(x.to(DEV), labels, tl, ll, blank, "one")
    assert st == 0
    assert np.isnan(c[1]) and np.isnan(g[1][mask[1]]).all() and not g[~mask].any()
    keep = [0, 2]
    rc, rg = _reference(x[keep], labels[keep], tl[keep], ll[keep], blank)
    _check("f32", c[keep], g[keep], rc, rg, mask[keep], labels[keep], ll[keep], blank, what="unpoisoned")
    from warprnnt_pytorch.hat import rnnt_loss_hat
    with pytest.raises(ValueError, match="blank"):
        rnnt_loss_hat(torch.nan_to_num(x).to(DEV), *dev(labels, tl, ll), blank=blank, reduction="none")


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_non_finite_inputs(dtype):
    """NaN in an in-lattice row (label or blank column), a +inf label logit, all label logits -inf: that sample only.
    z_blank = -inf / +inf are limits: finite cost while a path is left, +inf when none is."""
    N, T, U, A, blank = 8, 5, 3, 11, 6
    rng = np.random.default_rng(5)
    tl, ll = np.full(N, 4, np.int32), np.full(N, 2, np.int32)
    tl[0] = 5
    x, labels, tl, ll, mask = _problem("nf_" + dtype, dtype, N, T, U, A, blank, rng=rng, lengths=(tl, ll))
    inf = float("inf")
    x[1, 1, 0, 3] = float("nan")                                 # a NaN label logit
    x[2, 2, 1, blank] = float("nan")                             # a NaN blank logit
    x[3, 0, 1, 8] = inf                                          # a +inf label logit
    x[4, 0, 1, :] = -inf
    x[4, 0, 1, blank] = 0.5                                      # all label logits -inf
    x[5, 1, 1, blank] = -inf                                     # b = 0 in one cell: paths around it remain
    x[5, 2, 0, blank] = inf                                      # b = 1 in one cell
    x[6, 3, 2, blank] = -inf                                     # b = 0 in the terminal cell: no path
    x[7, :, 0:2, blank] = inf                                    # b = 1 wherever a label must be emitted: no path
    st, c, g = call(x.to(DEV), labels, tl, ll, blank, "one")
    assert st == 0
    for b in (1, 2, 3, 4):
        assert np.isnan(c[b]) and np.isnan(g[b][mask[b]]).all(), (b, c)
    for b in (6, 7):
        assert np.isposinf(c[b]), (b, c)
    assert not g[~mask].any()
    keep = [0, 5]
    # the reference takes the limits at z_blank = -200 / +200: autograd through logsigmoid(+-inf) is NaN, and sigmoid(+-200)
    # differs from 0 / 1 by e^-200, far below every bound here
    xr = x[keep].clone()
    xr[..., blank] = torch.nan_to_num(xr[..., blank].float(), nan=0.0).clamp(-200.0, 200.0).to(xr.dtype)
    rc, rg = _reference(xr, labels[keep], tl[keep], ll[keep], blank)
    assert np.isfinite(rc).all()
    _check(dtype, c[keep], g[keep], rc, rg, mask[keep], labels[keep], ll[keep], blank, what="limits")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_blank_logit_of_magnitude_80(dtype):
    """|z_blank| = 80: log(1 - sigmoid(80)) is -inf in fp32 arithmetic, -softplus(80) is -80."""
    N, T, U, A, blank = 2, 2, 2, 7, 3
    tl, ll = np.array([2, 2], np.int32), np.array([1, 1], np.int32)
    x, labels, tl, ll, mask = _problem("z80_" + dtype, dtype, N, T, U, A, blank, lengths=(tl, ll), scale=1.0)
    x[0, :, :, blank] = torch.tensor([[80.0, -80.0], [-80.0, 80.0]]).to(x.dtype)
    x[1, :, :, blank] = torch.tensor([[-80.0, 80.0], [80.0, -80.0]]).to(x.dtype)
    st, c, g = call(x.to(DEV), labels, tl, ll, blank, "one")
    assert st == 0 and np.isfinite(c).all() and c.max() > 70, c     # (sample 1 has to pay one 80 at least)
    rc, rg = _reference(x, labels, tl, ll, blank)
    assert np.isfinite(rc).all() and np.isfinite(rg).all()
    _check(dtype, c, g, rc, rg, mask, labels, ll, blank, what="z80")


def test_closed_form_single_cell():
    """T = 1, L = 0: cost = softplus(-z_blank)."""
    z = np.array([-3.0, 0.25, 7.0])
    x = torch.zeros((3, 1, 1, 4), dtype=torch.float64)
    x[:, 0, 0, 2] = torch.tensor(z)
    st, c, _ = call(x.to(DEV), np.zeros((3, 0), np.int32), np.ones(3, np.int32), np.zeros(3, np.int32), 2, "score")
    assert st == 0 and np.allclose(c, np.log1p(np.exp(-z)), rtol=1e-12)


def test_cross_check_against_rnntloss_of_hat_log_probs():
    """HATLoss(z) against RNNTLoss(hat_log_probs(z)) with autograd through the transform, fp64, on the GPU."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.hat import HATLoss, hat_log_probs
    N, T, U, A, blank = 4, 12, 8, 37, 9
    rng = np.random.default_rng(17)
    tl, ll = ragged_lengths(N, T, U, rng)
    tl[1] = 3
    labels = _labels(rng, N, U, A, blank)
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * 2, dtype=torch.float64, device=DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    xa = x.clone().requires_grad_()
    la = HATLoss(blank=blank, reduction="none")(xa, lab, ttl, tll)
    la.sum().backward()
    xb = x.clone().requires_grad_()
    lb = RNNTLoss(blank=blank, reduction="none")(hat_log_probs(xb, blank), lab, ttl, tll)
    lb.sum().backward()
    assert torch.allclose(la, lb, rtol=1e-9, atol=1e-9), (la, lb)
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    ga, gb = xa.grad.cpu().numpy(), xb.grad.cpu().numpy()
    assert not ga[~mask].any()
    O.assert_grads(ga[mask], gb[mask], _mag(gb, labels, ll, blank)[mask], torch.float64, what="cross-check")


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_reductions(reduction):
    from warprnnt_pytorch.hat import HATLoss
    N, T, U, A, blank = 3, 6, 4, 11, 10
    rng = np.random.default_rng(3)
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 1], np.int32)
    x, labels, tl, ll, mask = _problem("ag", "f32", N, T, U, A, blank, rng=rng, lengths=(tl, ll))
    x = torch.nan_to_num(x)
    xd = x.to(DEV).requires_grad_()
    loss = HATLoss(blank=blank, reduction=reduction)(xd, *dev(labels, tl, ll))
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
    from warprnnt_pytorch.hat import rnnt_loss_hat
    N, T, U, A, blank = 2, 4, 3, 5, 2
    rng = np.random.default_rng(2)
    labels = _labels(rng, N, U, A, blank)
    lab, ttl, tll = dev(labels, np.array([4, 3], np.int32), np.array([2, 1], np.int32))
    x = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda z: rnnt_loss_hat(z, lab, ttl, tll, blank, "none"), (x,), eps=1e-6, atol=1e-6,
                                    nondet_tol=1e-12)


def test_cpu_tensors_are_refused():
    from warprnnt_pytorch.hat import rnnt_loss_hat
    x = torch.zeros(1, 2, 2, 5)
    with pytest.raises(ValueError, match="GPU"):
        rnnt_loss_hat(x, torch.ones(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                      torch.tensor([1], dtype=torch.int32))


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch), replayed on new logits."""
    from warprnnt_pytorch.hat import rnnt_loss_hat
    N, T, U, A, blank = 3, 8, 5, 33, 32
    rng = np.random.default_rng(11)
    tl, ll = np.array([8, 6, 4], np.int32), np.array([4, 0, 2], np.int32)
    labels = _labels(rng, N, U, A, blank)
    lab, ttl, tll = dev(labels, tl, ll)
    static_x = torch.zeros((N, T, U, A), device=DEV, requires_grad=True)
    h = _hat()
    h.lib()
    h.workspace_bytes(T, U, N, 0)

    def step():
        static_x.grad = None
        loss = rnnt_loss_hat(static_x, lab, ttl, tll, blank, "sum", validate=False)
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
        loss = rnnt_loss_hat(static_x, lab, ttl, tll, blank, "sum", validate=False)
        loss.backward()
    grad = static_x.grad
    for seed in (1, 2):
        xn = np.random.default_rng(seed).standard_normal((N, T, U, A)).astype(np.float32)
        with torch.no_grad():
            static_x.copy_(torch.tensor(xn))
        graph.replay()
        torch.cuda.synchronize()
        rc, rg = R.hat_autograd(xn, labels, tl, ll, blank)
        assert abs(loss.item() - rc.sum()) < 1e-5 * rc.sum()
        mask = R.in_lattice_mask((N, T, U), tl, ll)
        got = grad.double().cpu().numpy()
        assert not got[~mask].any()
        O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, blank)[mask], torch.float32, what="replay %d" % seed)


# ----------------------------------------------------------------------------- c3- and c4-shaped problems
@pytest.mark.parametrize("shape", ["c3", "c4"])
def test_benchmark_shapes(shape):
    """Two samples at the c3 shape (T = 150, U = 21, A = 5000) and the c4 shape (T = 1500, U = 301, A = 50: lattice_kernel
    with 1800 anti-diagonals), fp32, ragged."""
    T, U, A, blank = (150, 21, 5000, 0) if shape == "c3" else (1500, 301, 50, 49)
    N = 2
    rng = np.random.default_rng(7)
    tl, ll = np.array([T, (3 * T) // 4], np.int32), np.array([U - 1, (5 * U) // 6], np.int32)
    x, labels, tl, ll, mask = _problem(shape, "f32", N, T, U, A, blank, rng=rng, lengths=(tl, ll), scale=1.0)
    st, c, g = call(x.to(DEV), labels, tl, ll, blank, "one")
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, blank)
    assert np.isfinite(rc).all()
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, what=shape)


# ----------------------------------------------------------------------------- the record table's overlay (launch_coef)
@pytest.mark.parametrize("form,U", [("cell", 48), ("tiled", 49)])
def test_record_table_overlays_the_lattice_blocks(form, U):
    """A record table past 32 MB (rnnt_host.h, make_layout) through the shared coefficient launcher: at maxU = 48 the
    cell-per-thread kernel in groups of samples (N = 40 > group = 39: two launches, the second one's records on sample 0's
    block), at maxU = 49 ONE launch of the tiled kernel with its overlay guard live (group = 38 < N).  No case of
    tests/hat_forms.py reaches either: their tables are a few KB."""
    from tests import kernel_forms as K
    N, T, A, blank = 40, 1100, 3, 0
    rec1 = T * U * 16
    assert N * rec1 > K.ONE_GROUP_BYTES and K.ONE_GROUP_BYTES // rec1 == (39 if form == "cell" else 38)
    groups = K.coef_launches(dict(dtype="f32", N=N, T=T, U=U, A=A), G.cus())       # (make_layout's group < N)
    assert groups == 2
    rng = np.random.default_rng(zlib.crc32(("overlay_" + form).encode()))
    # Which records land on which block depends on maxT, maxU and N alone (every sample's T x U records are written, padding
    # rows included): sample 0, whose block they land on, and the last sample, whose records do, are full; the others stay
    # under 96 frames so that the fp64 reference (a Python loop over frames) takes a second
    tl, ll = ragged_lengths(N, T, U, rng)
    tl[1:-1] = np.minimum(tl[1:-1], rng.integers(1, 97, size=N - 2))
    tl[-1], ll[-1] = T, U - 1
    x, labels, tl, ll, mask = _problem("overlay_" + form, "f32", N, T, U, A, blank, rng=rng, lengths=(tl, ll))
    gv = torch.full_like(x, float("nan")).to(DEV)
    (st, c, g), names = profiled(lambda: call(x.to(DEV), labels, tl, ll, blank, "one", grads=gv))
    assert st == 0
    coef = [n for n in names if F.stage_of(n) == "coef"]
    want = ["rnnt::coef_cell_kernel<float>"] * groups if form == "cell" else ["rnnt::coef_kernel<float, false>"]
    assert coef == want, coef
    rc, rg = _reference(x, labels, tl, ll, blank)
    _check("f32", c, g, rc, rg, mask, labels, ll, blank, what="overlay " + form)


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_in_place_past_2_31_elements():
    """bf16 in place, N T U A > 2^31 elements: the last sample's in-lattice rows lie past element 2^31."""
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
    labels = _labels(rng, N, U, A, blank)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((N, T, U, A), generator=g, device=DEV, dtype=torch.bfloat16)
    small = torch.zeros((N, 4, 4, A), dtype=torch.float64)
    for b in range(N):
        small[b, :tl[b], :ll[b] + 1] = x[b, :tl[b], :ll[b] + 1].double().cpu()
    st, c, _ = call(x, labels, tl, ll, blank, "inplace")
    assert st == 0
    rc, rg = R.hat_autograd(small.numpy(), labels[:, :3], tl, ll, blank)
    assert np.allclose(c, rc, rtol=1e-5, atol=1e-5), (c, rc)
    for b in range(N):
        assert x[b, tl[b]:].count_nonzero().item() == 0
        assert x[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
        got = x[b, :tl[b], :ll[b] + 1].double().cpu().numpy()
        ref = rg[b, :tl[b], :ll[b] + 1]
        O.assert_grads(got, ref, np.maximum(np.abs(ref), np.abs(ref).sum(-1, keepdims=True)), torch.bfloat16,
                       what="sample %d" % b)
