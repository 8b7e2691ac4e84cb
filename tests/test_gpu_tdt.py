"""-m gpu: the Token-and-Duration Transducer loss (include/rnnt_tdt.h, libwarprnnt_tdt.so).

Every case of tests/tdt_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules predict run,
stage by stage.  Costs and gradients are compared with the fp64 autograd reference of tests/tdt_ref.py at the per-dtype bounds
of oracle.grad_bound; ragged lengths (one sample with T_b = 1, one with L_b = 0), NaN in every padding row (never read) and
gradient buffers that start as NaN (padding must come back as exact zeros).  Then the call forms, the invalid arguments, the
samples without a path and the poisoned rows, the autograd module, and one bf16 tensor past 2^31 elements."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import tdt_forms as F
from tests import tdt_ref as R
from tests.gpu_support import (CODE, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check, dev,
                               options, place, profiled, ragged_lengths, stages_seen)

pytestmark = pytest.mark.gpu


def _tdt():
    from warprnnt_pytorch import tdt
    return tdt


def _problem(name, dtype, N, T, U, A, durations, rng=None, lengths=None, scale=2.0):
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = lengths if lengths is not None else ragged_lengths(N, T, U, rng)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    x = torch.tensor(rng.standard_normal((N, T, U, A + len(durations))) * scale, dtype=torch.float32).to(TORCH[dtype])
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    x[torch.tensor(~mask)] = float("nan")
    return x, labels, tl, ll, mask


def call(x, labels, tl, ll, durations, form="one", scale=None, grads=None, blank=0, sigma=0.0, stream=None, ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host."""
    t = _tdt()
    N, T, U, W = x.shape
    D = len(durations)
    A = W - D
    code = CODE[NAME[x.dtype]]
    lab, ttl, tll = dev(labels if labels.size else np.zeros((N, 1), np.int32), tl, ll)
    dur = (C.c_int * D)(*durations)
    opt = options(T, U, blank, stream)
    lib = t.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    return call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_tdt_loss(x.data_ptr(), gp, dur, D, sigma, *lens, costs, ws, opt, code),
        lambda costs, ws: lib.compute_tdt_loss_fwd(x.data_ptr(), dur, D, sigma, *lens, costs, ws, opt, code, 1),
        lambda gp, sc, ws: lib.compute_tdt_loss_bwd(x.data_ptr(), gp, sc, dur, D, A, N, ws, opt, code),
        t.workspace_bytes(T, U, N, D, code), scale, grads, stream, ws)


def _reference(x, labels, tl, ll, durations, blank=0, sigma=0.0, weights=None):
    xr = torch.nan_to_num(x.double().cpu(), nan=0.0).numpy()
    return R.tdt_autograd(xr, labels, tl, ll, durations, blank, sigma, weights)


def _mag(ref, labels, ll, A, blank):
    """The size of the terms of every gradient element: |ref|, and for the blank and label columns and the duration columns
    the row's |ref| sum (they carry the subtracted posteriors)."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    mag[..., blank] = np.maximum(mag[..., blank], rs)
    mag[..., A:] = np.maximum(mag[..., A:], rs[..., None])
    N, T, U, _ = ref.shape
    for b in range(N):
        for u in range(min(U, int(ll[b]))):
            lab = int(labels[b, u])
            mag[b, :, u, lab] = np.maximum(mag[b, :, u, lab], rs[b, :, u])
    return mag


def _check(dtype, got_c, got_g, ref_c, ref_g, mask, labels, ll, A, blank=0, scale=None, what=""):
    check(dtype, got_c, got_g, ref_c, ref_g, mask, lambda ref, b: _mag(ref, labels[b:b + 1], ll[b:b + 1], A, blank), scale, what,
          diagonals=mask.shape[1] + labels.shape[1])


def _assert_real(c, ll, what):
    """Not only +inf: some sample with labels came out finite."""
    assert any(np.isfinite(c[b]) and ll[b] > 0 for b in range(len(c))), (what, c, ll)


# ----------------------------------------------------------------------------- every form of tests/tdt_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_tdt_form(name):
    case = F.CASES[name]
    cus = G.cus()
    N, T, U, A, durs, dtype = case["N"], case["T"], case["U"], case["A"], case["durations"], case["dtype"]
    x, labels, tl, ll, mask = _problem(name, dtype, N, T, U, A, durs)
    off = case.get("off", 0)
    xv = place(x.to(DEV), off, x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, durs, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, cus))
    rc, rg = _reference(x, labels, tl, ll, durs)
    _assert_real(c, ll, name)
    _check(dtype, c, g, rc, rg, mask, labels, ll, A, what=name)


def test_every_tdt_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- parity against the fp64 reference
_SETS = [(0, 1, 2, 3, 4), (0, 1, 2, 4, 8), (0, 2, 4), (1, 2), (1,), (1, 2, 3)]
_SHAPES = [  # N, T, U, A, durations (sets without 0 need T_b > L_b)
    (4, 6, 1, 2, (0, 1, 2, 3, 4)), (4, 7, 2, 65, (0, 1, 2, 4, 8)), (3, 10, 17, 1025, (0, 2, 4)), (3, 10, 9, 5000, (1, 2)),
    (2, 70, 65, 2, (1,)), (2, 8, 300, 65, (0, 1, 2, 3, 4)), (2, 4, 601, 2, (0, 1, 2, 4, 8))]


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("shape", range(len(_SHAPES)))
def test_parity(dtype, shape):
    N, T, U, A, durs = _SHAPES[shape]
    blank = A - 1 if shape % 2 else 0
    sigma = 0.05 if shape % 3 == 1 else 0.0
    name = "par_%s_%d" % (dtype, shape)
    x, labels, tl, ll, mask = _problem(name, dtype, N, T, U, A, durs)
    st, c, g = call(x.to(DEV), labels, tl, ll, durs, "one", blank=blank, sigma=sigma)
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, durs, blank, sigma)
    if U > 1:
        _assert_real(c, ll, name)
    _check(dtype, c, g, rc, rg, mask, labels, ll, A, blank, what=name)


@pytest.mark.parametrize("durs", _SETS)
def test_parity_duration_sets(durs):
    N, T, U, A = 4, 11, 6, 33
    x, labels, tl, ll, mask = _problem("sets_%s" % (durs,), "f32", N, T, U, A, durs)
    for blank, sigma in ((0, 0.0), (A - 1, 0.05)):
        st, c, g = call(x.to(DEV), labels, tl, ll, durs, "one", blank=blank, sigma=sigma)
        assert st == 0
        rc, rg = _reference(x, labels, tl, ll, durs, blank, sigma)
        _check("f32", c, g, rc, rg, mask, labels, ll, A, blank, what=str(durs))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_parity_long(dtype):
    """Near c4: T = 1500, U = 301 (1800 anti-diagonals), ragged."""
    N, T, U, A = 2, 1500, 301, 3
    durs = (0, 1, 2, 3, 4)
    rng = np.random.default_rng(7)
    tl, ll = np.array([T, 1100], np.int32), np.array([U - 1, 250], np.int32)
    x, labels, tl, ll, mask = _problem("long_" + dtype, dtype, N, T, U, A, durs, rng=rng, lengths=(tl, ll), scale=1.0)
    st, c, g = call(x.to(DEV), labels, tl, ll, durs, "one", blank=A - 1)
    assert st == 0
    rc, rg = _reference(x, labels, tl, ll, durs, A - 1)
    assert np.isfinite(rc).all()
    _check(dtype, c, g, rc, rg, mask, labels, ll, A, A - 1, what="long")


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_call_forms_agree(dtype):
    N, T, U, A = 5, 7, 9, 130
    durs = (0, 1, 2, 3, 4)
    x, labels, tl, ll, mask = _problem("forms_" + dtype, dtype, N, T, U, A, durs)
    xd = x.to(DEV)
    st, c1, g1 = call(xd, labels, tl, ll, durs, "one")
    assert st == 0
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    st, c2, g2 = call(xd, labels, tl, ll, durs, "two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    rc, rg = _reference(x, labels, tl, ll, durs, weights=scale)
    _check(dtype, c2, g2, rc, rg / 1.0, mask, labels, ll, A, scale=None, what="two-phase")
    g1s = g1 * scale[:, None, None, None]
    assert np.allclose(g2, g1s, rtol=1e-2 if dtype == "bf16" else 1e-6, atol=1e-6)
    xi = xd.clone()
    st, c3, g3 = call(xi, labels, tl, ll, durs, "inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1)
    st, c4, _ = call(xd, labels, tl, ll, durs, "score")
    assert st == 0 and np.array_equal(c1, c4)
    st, c5, g5 = call(xd, labels, tl, ll, durs, "host", grads=torch.full_like(xd, float("nan")))
    assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5)


def test_invalid_arguments():
    t = _tdt()
    N, T, U, A = 2, 4, 3, 5
    x, labels, tl, ll, _ = _problem("inv", "f32", N, T, U, A, (0, 1, 2))
    xd = x.to(DEV)
    for durs in ((), (1, 1), (2, 1), (-1, 1), (0,), (0, 65), tuple(range(9))):
        D = len(durs)
        dur = (C.c_int * max(D, 1))(*durs)
        lab, ttl, tll = dev(labels, tl, ll)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        costs = np.zeros(N, np.float32)
        st = t.lib().compute_tdt_loss(xd.data_ptr(), None, dur, D, 0.0, lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(),
                                      x.shape[3] - D, N, costs.ctypes.data, ws.data_ptr(), options(T, U), 0)
        assert st == 2, durs
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed
    st, c, _ = call(xd, labels, np.array([T + 1, T], np.int32), ll, (0, 1, 2), "host")
    assert st == 2
    st, c, g = call(torch.nan_to_num(xd), labels, np.array([T, T], np.int32), np.array([U, 1], np.int32), (0, 1, 2), "one")
    assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any()
    # blank outside the token columns, maxU past the limit
    st, _, _ = call(xd, labels, tl, ll, (0, 1, 2), "one", blank=A)
    assert st == 2
    xb = torch.zeros((1, 1, 4097, 3), device=DEV)
    st, _, _ = call(xb, np.zeros((1, 4096), np.int32), np.array([1], np.int32), np.array([0], np.int32), (1,), "one")
    assert st == 2


def test_no_path_and_poison_stay_isolated():
    N, T, U, A = 4, 5, 3, 6
    durs = (0, 2)
    rng = np.random.default_rng(5)
    # sample 1: L_b = 0 and odd T_b: only even frames are reachable, the final blank needs T_b - 2 even -> no path
    tl, ll = np.array([4, 3, 4, 4], np.int32), np.array([2, 0, 1, 2], np.int32)
    x, labels, tl, ll, mask = _problem("iso", "f32", N, T, U, A, durs, rng=rng, lengths=(tl, ll))
    x[2, 1, 0, 3] = float("nan")                                 # sample 2: a poisoned in-lattice row
    x[3, 0, 1, :A] = -float("inf")                               # sample 3: an all -inf token part
    st, c, g = call(x.to(DEV), labels, tl, ll, durs, "one")
    assert st == 0
    assert np.isposinf(c[1]) and np.isnan(g[1][mask[1]]).all()
    assert np.isnan(c[2]) and np.isnan(g[2][mask[2]]).all()
    assert np.isnan(c[3]) and np.isnan(g[3][mask[3]]).all()
    assert not g[~mask].any()
    rc, rg = _reference(x[:1], labels[:1], tl[:1], ll[:1], durs)
    _check("f32", c[:1], g[:1], rc, rg, mask[:1], labels[:1], ll[:1], A, what="isolated")


def test_single_duration_closed_form():
    """durations = [1], T_b = L_b + 1: one path -- the labels on the diagonal, then the final blank."""
    N, T, U, A = 2, 6, 6, 7
    rng = np.random.default_rng(9)
    tl, ll = np.array([6, 4], np.int32), np.array([5, 3], np.int32)
    x, labels, tl, ll, mask = _problem("one", "f64", N, T, U, A, (1,), rng=rng, lengths=(tl, ll))
    st, c, _ = call(x.to(DEV), labels, tl, ll, (1,), "one")
    assert st == 0
    xn = torch.nan_to_num(x).numpy()
    for b in range(N):
        L = int(ll[b])
        lp = torch.log_softmax(torch.tensor(xn[b, :, :, :A]), -1).numpy()
        want = -(sum(lp[u, u, labels[b, u]] for u in range(L)) + lp[L, L, 0])
        assert abs(c[b] - want) < 1e-9 * max(1.0, abs(want)), (b, c[b], want)


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_reductions(reduction):
    from warprnnt_pytorch.tdt import TDTLoss
    N, T, U, A = 3, 6, 4, 11
    durs = (0, 1, 2, 4)
    rng = np.random.default_rng(3)
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 1], np.int32)
    x, labels, tl, ll, mask = _problem("ag", "f32", N, T, U, A, durs, rng=rng, lengths=(tl, ll))
    x = torch.nan_to_num(x)
    xd = x.to(DEV).requires_grad_()
    loss = TDTLoss(durs, blank=A - 1, sigma=0.05, reduction=reduction)(xd, *dev(labels, tl, ll))
    go = torch.tensor([0.7, -1.3, 2.0][:loss.numel()], device=DEV).view(loss.shape)
    (loss * go).sum().backward()
    w = go.detach().cpu().numpy().reshape(-1)
    w = np.broadcast_to(w, (N,)) / (N if reduction == "mean" else 1)
    rc, rg = _reference(x, labels, tl, ll, durs, A - 1, 0.05, weights=w)
    want = {"none": rc, "sum": rc.sum(keepdims=True), "mean": rc.mean(keepdims=True)}[reduction]
    assert np.allclose(loss.detach().cpu().numpy(), want, rtol=1e-5)
    got = xd.grad.double().cpu().numpy()
    assert not got[~mask].any()
    O.assert_grads(got[mask], rg[mask], _mag(rg, labels, ll, A, A - 1)[mask], torch.float32)


def test_backward_through_a_joiner():
    from warprnnt_pytorch.tdt import rnnt_loss_tdt
    N, T, U, A, H = 2, 5, 4, 9, 8
    durs = (0, 1, 2)
    torch.manual_seed(0)
    enc = torch.randn(N, T, H, dtype=torch.float64)
    pred = torch.randn(N, U, H, dtype=torch.float64)
    lin = torch.nn.Linear(H, A + len(durs)).double()
    labels = torch.randint(0, A - 1, (N, U - 1), dtype=torch.int32)
    tl, ll = torch.tensor([5, 4], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)

    j_dev = torch.nn.Linear(H, A + len(durs)).double().to(DEV)
    j_dev.load_state_dict(lin.state_dict())
    logits = j_dev(torch.tanh(enc.to(DEV)[:, :, None] + pred.to(DEV)[:, None]))
    loss = rnnt_loss_tdt(logits, labels.to(DEV), tl.to(DEV), ll.to(DEV), durs, blank=A - 1, reduction="sum")
    loss.backward()
    logits_ref = lin(torch.tanh(enc[:, :, None] + pred[:, None]))
    c, g = R.tdt_autograd(logits_ref.detach().numpy(), labels.numpy(), tl.numpy(), ll.numpy(), durs, A - 1)
    logits_ref.backward(torch.tensor(g))
    assert abs(loss.item() - c.sum()) < 1e-9 * max(1.0, c.sum())
    assert torch.allclose(j_dev.weight.grad.cpu(), lin.weight.grad, rtol=1e-8, atol=1e-10)
    assert torch.allclose(j_dev.bias.grad.cpu(), lin.bias.grad, rtol=1e-8, atol=1e-10)


def test_cpu_tensors_are_refused():
    from warprnnt_pytorch.tdt import rnnt_loss_tdt
    x = torch.zeros(1, 2, 2, 5)
    with pytest.raises(ValueError, match="GPU"):
        rnnt_loss_tdt(x, torch.zeros(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                      torch.tensor([1], dtype=torch.int32), (0, 1))


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_in_place_past_2_31_elements():
    """bf16 in place, N T U W > 2^31 elements: the last sample's in-lattice rows lie past element 2^31."""
    N, T, U, A = 5, 64, 65, 130000
    durs = (0, 1, 2, 3, 4)
    W = A + len(durs)
    E = N * T * U * W
    assert E > 2 ** 31 and 4 * T * U * W > 2 ** 31 - 3 * T * U * W
    tl, ll = np.array([1, 2, 3, 2, 4], np.int32), np.array([0, 1, 2, 1, 3], np.int32)
    rng = np.random.default_rng(13)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((N, T, U, W), generator=g, device=DEV, dtype=torch.bfloat16)
    small = torch.zeros((N, 4, 4, W), dtype=torch.float64)
    for b in range(N):
        small[b, :tl[b], :ll[b] + 1] = x[b, :tl[b], :ll[b] + 1].double().cpu()
    st, c, _ = call(x, labels, tl, ll, durs, "inplace")
    assert st == 0
    rc, rg = R.tdt_autograd(small.numpy(), labels[:, :3], tl, ll, durs)
    assert np.allclose(c, rc, rtol=1e-5, atol=1e-5), (c, rc)
    for b in range(N):
        assert x[b, tl[b]:].count_nonzero().item() == 0
        assert x[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
        got = x[b, :tl[b], :ll[b] + 1].double().cpu().numpy()
        ref = rg[b, :tl[b], :ll[b] + 1]
        O.assert_grads(got, ref, np.maximum(np.abs(ref), np.abs(ref).sum(-1, keepdims=True)), torch.bfloat16,
                       what="sample %d" % b)
