"""-m gpu: the transducer lattice distillation loss (include/rnnt_kd.h, libwarprnnt_kd.so).

Every case of tests/kd_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules predict run,
stage by stage.  Student and teacher are independent N(0, 1) * 2 logits; ragged lengths (one sample with T_b = 1, one with
L_b = 0), NaN in every padding row of BOTH tensors (never read) and gradient buffers that start as NaN (padding must come back
as exact zeros).

Costs are held to |got - ref| <= COST_TOL[dtype] * mag_b + COST_TOL[dtype] against the fp64 reference of tests/kd_ref.py, mag_b
the size of the cost's terms (kd_ref.cost_mag): the KL itself can be 50 times smaller than its terms.  Gradients per element at
oracle.grad_bound with mag = (p_v + p_v Q / P) / tau, scaled.  Negative controls compare the collapsed result with the full
reference and the result with the reference of swapped operands, and must fail.  Then the call forms, bit-identical runs, the
temperatures, rows of two classes, every refusal of the header, the non-finite cases, the autograd module against
kd_loss_torch, a HIP-graph capture and one bf16 problem past 2^31 elements."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import kd_forms as F
from tests import kd_ref as R
from tests.gpu_support import (CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, dev,
                               options, place, profiled, ragged_lengths, stages_seen)

pytestmark = pytest.mark.gpu
_BOUND_DTYPE = {"f32": "float32", "f64": "float64", "bf16": "bfloat16", "f16": "float16"}     # oracle.grad_bound's names


def _kd():
    from warprnnt_pytorch import kd
    return kd


def _problem(name, dtype, N, T, U, A, blank, rng=None, lengths=None, scale=2.0):
    """Independent student and teacher logits, NaN in the padding rows of both; labels anywhere in [0, A)."""
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = lengths if lengths is not None else ragged_lengths(N, T, U, rng)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    out = []
    for _ in range(2):
        x = torch.tensor(rng.standard_normal((N, T, U, A)) * scale, dtype=torch.float32).to(TORCH[dtype])
        x[torch.tensor(~mask)] = float("nan")
        out.append(x)
    return out[0], out[1], labels, tl, ll, mask


def call(z, w, labels, tl, ll, blank=0, mode=0, tau=1.0, form="one", scale=None, grads=None, stream=None, ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host.  z, w on the device."""
    k = _kd()
    N, T, U, A = z.shape
    code = CODE[NAME[z.dtype]]
    lab, ttl, tll = dev(labels if labels.size else np.zeros((N, 1), np.int32), tl, ll)
    opt = options(T, U, blank, stream)
    lib = k.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    tau = ctypes.c_float(tau)
    return call_forms(
        z, form,
        lambda gp, costs, ws: lib.compute_kd_loss(z.data_ptr(), w.data_ptr(), gp, *lens, costs, ws, opt, code, mode, tau),
        lambda costs, ws: lib.compute_kd_loss_fwd(z.data_ptr(), w.data_ptr(), *lens, costs, ws, opt, code, mode, tau, 1),
        lambda gp, sc, ws: lib.compute_kd_loss_bwd(z.data_ptr(), w.data_ptr(), gp, sc, A, N, ws, opt, code, mode, tau),
        k.workspace_bytes(T, U, N, code), scale, grads, stream, ws)


def _f64(x):
    return torch.nan_to_num(x.double().cpu(), nan=0.0, posinf=float("inf"), neginf=float("-inf")).numpy()


class Ref:
    """The fp64 reference of one problem: costs, gradients (scaled) and the sizes of their terms."""

    def __init__(self, z, w, labels, tl, ll, blank=0, mode=0, tau=1.0, weights=None):
        args = (_f64(z), _f64(w), labels, tl, ll, blank, mode, tau)
        self.wts = np.ones(len(tl)) if weights is None else np.asarray(weights, np.float64)
        self.c, self.g = R.kd_autograd(*args, weights=self.wts)
        self.cmag = R.cost_mag(*args)
        self.gmag = R.grad_mag(*args) * np.abs(self.wts)[:, None, None, None]
        self.mask = R.in_lattice_mask(z.shape, tl, ll)


def check_costs(dtype, got, ref, what=""):
    """|got - ref| <= COST_TOL * mag_b + COST_TOL; returns the worst error / bound."""
    tol = COST_TOL[dtype]
    bound = tol * ref.cmag + tol
    ratio = np.abs(np.asarray(got, np.float64) - ref.c) / bound
    print(what, "max cost error / bound = %.4f (max |cost| %.3g, max mag %.3g)" % (ratio.max(), np.abs(ref.c).max(), ref.cmag.max()))
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), (what, got, ref.c, bound)
    return float(ratio.max())


def check_grads(dtype, got, ref, what=""):
    """Padding exact zeros; every in-lattice element at oracle.grad_bound with mag = the sum of its two terms' sizes."""
    assert not got[~ref.mask].any(), (what, "padding must be exact zeros")
    worst = 0.0
    for b in range(len(ref.c)):
        m = ref.mask[b]
        r = O.grad_check(got[b][m], ref.g[b][m], ref.gmag[b][m], _BOUND_DTYPE[dtype])
        worst = max(worst, r["max_err_over_quantum"])
        assert r["passed"], ("%s sample %d" % (what, b), r)
    print(what, "max gradient error / bound = %.3f" % worst)
    return worst


def _check(dtype, c, g, ref, what=""):
    check_costs(dtype, c, ref, what)
    if g is not None:
        check_grads(dtype, g, ref, what)


# ----------------------------------------------------------------------------- every form of tests/kd_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_kd_form(name):
    case = F.CASES[name]
    N, T, U, A, blank, dtype, mode = case["N"], case["T"], case["U"], case["A"], case["blank"], case["dtype"], case["mode"]
    z, w, labels, tl, ll, mask = _problem(name, dtype, N, T, U, A, blank)
    off, toff = case.get("off", 0), case.get("off", 0) + case.get("toff", 0)
    zv, wv = place(z.to(DEV), off, z.dtype), place(w.to(DEV), toff, w.dtype)
    gv = place(torch.full_like(z, float("nan")).to(DEV), off, z.dtype)

    (st, c, g), names = profiled(lambda: call(zv, wv, labels, tl, ll, blank, mode, 1.0, "one", grads=gv))
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case))
    _check(dtype, c, g, Ref(z, w, labels, tl, ll, blank, mode), what=name)


def test_every_kd_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_negative_controls_are_refused(dtype):
    """The collapsed result against the full reference, and the result against the reference with student and teacher
    swapped, must fail: the checks cannot pass on another loss."""
    N, T, U, A, blank = 4, 9, 7, 40, 13
    z, w, labels, tl, ll, mask = _problem("neg_" + dtype, dtype, N, T, U, A, blank)
    st, c, g = call(z.to(DEV), w.to(DEV), labels, tl, ll, blank, 0)
    assert st == 0
    _check(dtype, c, g, Ref(z, w, labels, tl, ll, blank, 0), what="collapsed")
    for other in (Ref(z, w, labels, tl, ll, blank, 1), Ref(w, z, labels, tl, ll, blank, 0)):
        with pytest.raises(AssertionError):
            check_costs(dtype, c, other, what="control costs")
        with pytest.raises(AssertionError):
            check_grads(dtype, g, other, what="control gradients")


# ----------------------------------------------------------------------------- call forms and edge cases
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_call_forms_agree_and_runs_are_bit_identical(dtype, mode):
    N, T, U, A, blank = 5, 7, 9, 130, 77
    z, w, labels, tl, ll, mask = _problem("forms_%s_%d" % (dtype, mode), dtype, N, T, U, A, blank)
    zd, wd = z.to(DEV), w.to(DEV)
    st, c1, g1 = call(zd, wd, labels, tl, ll, blank, mode)
    assert st == 0
    st, c1b, g1b = call(zd, wd, labels, tl, ll, blank, mode)
    assert st == 0 and c1.tobytes() == c1b.tobytes() and g1.tobytes() == g1b.tobytes()      # two runs, identical bits
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    scale[3] = -1.5
    st, c2, g2 = call(zd, wd, labels, tl, ll, blank, mode, form="two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    _check(dtype, c2, g2, Ref(z, w, labels, tl, ll, blank, mode, weights=scale), what="two-phase")
    assert np.allclose(g2, g1 * scale[:, None, None, None], rtol=1e-2 if dtype == "bf16" else 1e-6, atol=1e-6)
    zi = zd.clone()
    st, c3, g3 = call(zi, wd, labels, tl, ll, blank, mode, form="inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(g3, g1)
    st, c4, _ = call(zd, wd, labels, tl, ll, blank, mode, form="score")
    assert st == 0 and np.array_equal(c1, c4)
    st, c5, g5 = call(zd, wd, labels, tl, ll, blank, mode, form="host", grads=torch.full_like(zd, float("nan")))
    assert st == 0 and np.array_equal(c1.astype(c5.dtype), c5) and np.array_equal(g5, g1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tau", [0.5, 2.0])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_temperatures(dtype, tau, mode):
    N, T, U, A, blank = 3, 6, 5, 70, 69
    z, w, labels, tl, ll, mask = _problem("tau_%s" % dtype, dtype, N, T, U, A, blank)
    st, c, g = call(z.to(DEV), w.to(DEV), labels, tl, ll, blank, mode, tau)
    assert st == 0
    ref = Ref(z, w, labels, tl, ll, blank, mode, tau)
    _check(dtype, c, g, ref, what="tau %g" % tau)
    with pytest.raises(AssertionError):            # ... and not the loss at temperature 1
        check_grads(dtype, g, Ref(z, w, labels, tl, ll, blank, mode, 1.0), what="control tau")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rows_of_two_classes_and_clamped_labels(dtype):
    """A label equal to the blank (inside L_b) makes its row one of two classes; labels outside [0, A) are clamped."""
    N, T, U, A, blank = 3, 5, 4, 9, 4
    tl, ll = np.array([5, 4, 5], np.int32), np.array([3, 2, 1], np.int32)
    z, w, labels, tl, ll, mask = _problem("two_" + dtype, dtype, N, T, U, A, blank, lengths=(tl, ll))
    labels[0, 1] = blank
    labels[1, 0], labels[1, 1] = -3, A + 7
    st, c, g = call(z.to(DEV), w.to(DEV), labels, tl, ll, blank, 0)
    assert st == 0
    _check(dtype, c, g, Ref(z, w, labels, tl, ll, blank, 0), what="two classes")
    clamped = labels.copy()
    clamped[1, 0], clamped[1, 1] = 0, A - 1
    st, c2, g2 = call(z.to(DEV), w.to(DEV), clamped, tl, ll, blank, 0)
    assert st == 0 and np.array_equal(c, c2) and np.array_equal(g, g2)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_teacher_is_the_student(dtype, mode):
    """teacher == activations (the same pointer): cost within the cost bound of 0, gradients within their bound of 0."""
    N, T, U, A, blank = 3, 6, 5, 300, 0
    z, _, labels, tl, ll, mask = _problem("self_" + dtype, dtype, N, T, U, A, blank)
    zd = z.to(DEV)
    st, c, g = call(zd, zd, labels, tl, ll, blank, mode)
    assert st == 0
    ref = Ref(z, z, labels, tl, ll, blank, mode)
    assert np.abs(ref.c).max() < 1e-12 and np.abs(ref.g).max() < 1e-12
    _check(dtype, c, g, ref, what="teacher == student")


def test_collapsed_backward_takes_no_teacher():
    """compute_kd_loss_bwd with teacher == NULL: the same bits in collapsed mode, refused in full mode."""
    N, T, U, A, blank = 3, 6, 5, 70, 69
    z, w, labels, tl, ll, mask = _problem("noteacher", "f32", N, T, U, A, blank)
    zd, wd = z.to(DEV), w.to(DEV)
    k = _kd()
    lab, ttl, tll = dev(labels, tl, ll)
    opt, tau = options(T, U, blank), ctypes.c_float(2.0)
    for mode in (0, 1):
        st, c, want = call(zd, wd, labels, tl, ll, blank, mode, 2.0, "two")
        assert st == 0
        ws = torch.empty(k.workspace_bytes(T, U, N, 0), dtype=torch.uint8, device=DEV)
        costs, g = torch.empty(N, device=DEV), torch.full_like(zd, float("nan"))
        assert k.lib().compute_kd_loss_fwd(zd.data_ptr(), wd.data_ptr(), lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N,
                                           costs.data_ptr(), ws.data_ptr(), opt, 0, mode, tau, 1) == 0
        st = k.lib().compute_kd_loss_bwd(zd.data_ptr(), None, g.data_ptr(), None, A, N, ws.data_ptr(), opt, 0, mode, tau)
        torch.cuda.synchronize()
        assert st == (0 if mode == 0 else 2)
        if mode == 0:
            assert np.array_equal(g.double().cpu().numpy(), want)


def test_refusals_of_the_header():
    N, T, U, A = 2, 4, 3, 5
    z, w, labels, tl, ll, _ = _problem("inv", "f32", N, T, U, A, 0)
    zd, wd = torch.nan_to_num(z.to(DEV)), torch.nan_to_num(w.to(DEV))
    # lengths that do not fit the tensor: the cost marker -> INVALID_VALUE with host costs; the other sample is computed
    st, c, _ = call(zd, wd, labels, np.array([T + 1, T], np.int32), ll, 0, form="host")
    assert st == 2
    for bad_tl, bad_ll in (([T + 1, T], [1, 1]), ([0, T], [1, 1]), ([T, T], [U, 1]), ([T, T], [-1, 1])):
        st, c, g = call(zd, wd, labels, np.array(bad_tl, np.int32), np.array(bad_ll, np.int32), 0)
        assert st == 0 and np.isnan(c[0]) and np.isfinite(c[1]) and not g[0].any() and g[1].any()
        assert c[:1].view(np.uint32)[0] == 0x7fc0dead                          # the marker of include/rnnt.h
    # mode, temperature, blank outside the columns, a single column, a dtype code
    for mode in (-1, 2):
        assert call(zd, wd, labels, tl, ll, 0, mode)[0] == 2
    for tau in (0.0, -2.0, float("inf"), float("nan")):
        for form in ("one", "score"):
            assert call(zd, wd, labels, tl, ll, 0, 0, tau, form)[0] == 2
    for blank in (A, -1):
        assert call(zd, wd, labels, tl, ll, blank)[0] == 2
    one = torch.zeros((1, 2, 1, 1), device=DEV)
    assert call(one, one.clone(), np.zeros((1, 0), np.int32), np.array([2], np.int32), np.array([0], np.int32))[0] == 2
    k = _kd()
    n = ctypes.c_size_t(0)
    assert k.lib().get_workspace_size_kd(4, 3, 1, 4, ctypes.byref(n)) == 2
    assert k.lib().get_workspace_size_kd(4, 5000, 1, 0, ctypes.byref(n)) == 0 and n.value > 0      # no limit on maxU
    # the three tensors: gradients over the activations without being them, on or over the teacher, a teacher that overlaps
    # the activations without being them; in place with the teacher being the activations too
    E = zd.numel()
    buf = torch.zeros(3 * E, device=DEV)
    a = buf[:E].view(zd.shape).copy_(zd)
    assert call(a, wd, labels, tl, ll, 0, grads=buf[4:4 + E].view(zd.shape))[0] == 2
    assert call(zd, a, labels, tl, ll, 0, grads=a)[0] == 2
    assert call(zd, a, labels, tl, ll, 0, grads=buf[4:4 + E].view(zd.shape))[0] == 2
    assert call(a, buf[4:4 + E].view(zd.shape), labels, tl, ll, 0)[0] == 2
    assert call(a, a, labels, tl, ll, 0, form="inplace")[0] == 2
    assert call(a, a, labels, tl, ll, 0, form="one")[0] == 0
    assert call(a, wd, labels, tl, ll, 0, form="inplace")[0] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
def test_non_finite_inputs(dtype, mode):
    """NaN or +inf in an in-lattice row of either tensor, or such a row all -inf in either: that sample only.  P(k) = 0 with
    Q(k) > 0 costs +inf with NaN gradients.  Q(k) = 0 is a limit: the class contributes nothing."""
    N, T, U, A, blank = 9, 5, 3, 11, 6
    rng = np.random.default_rng(5)
    tl, ll = np.full(N, 4, np.int32), np.full(N, 2, np.int32)
    tl[0] = 5
    z, w, labels, tl, ll, mask = _problem("nf_" + dtype, dtype, N, T, U, A, blank, rng=rng, lengths=(tl, ll))
    labels[:, 0] = 2                                             # (row u = 0: classes blank = 6, label = 2, rest)
    inf = float("inf")
    z[1, 1, 0, 3] = float("nan")                                 # a NaN student logit
    w[2, 2, 1, blank] = float("nan")                             # a NaN teacher logit
    z[3, 0, 1, 8] = inf                                          # a +inf student logit
    w[4, 3, 0, 2] = inf                                          # a +inf teacher logit
    z[5, 0, 2, :] = -inf                                         # a student row all -inf
    w[6, 1, 1, :] = -inf                                         # a teacher row all -inf
    z[7, 2, 0, blank] = -inf                                     # P(blank) = 0, Q(blank) > 0
    w[8, 1, 0, blank] = -inf                                     # Q(blank) = 0: contributes 0 ...
    w[8, 2, 0, 2] = -inf                                         # ... Q(label) = 0
    z[8, 3, 1, blank] = -inf
    w[8, 3, 1, blank] = -inf                                     # ... P(blank) = Q(blank) = 0
    st, c, g = call(z.to(DEV), w.to(DEV), labels, tl, ll, blank, mode)
    assert st == 0
    for b in (1, 2, 3, 4, 5, 6):
        assert np.isnan(c[b]) and np.isnan(g[b][mask[b]]).all(), (b, c)
    assert np.isposinf(c[7]) and np.isnan(g[7][mask[7]]).all(), c
    assert not g[~mask].any()
    keep = [0, 8]
    ref = Ref(z[keep], w[keep], labels[keep], tl[keep], ll[keep], blank, mode)
    assert np.isfinite(ref.c).all() and np.isfinite(ref.g).all()
    _check(dtype, c[keep], g[keep], ref, what="the other samples")


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("mode", ["collapsed", "full"])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_module_against_kd_loss_torch(reduction, mode):
    """TransducerKDLoss under every reduction with grad_output folded in, against kd_loss_torch on the GPU in fp64."""
    from warprnnt_pytorch.kd import TransducerKDLoss, kd_loss_torch
    N, T, U, A, blank, tau = 3, 6, 4, 11, 10, 2.0
    tl, ll = np.array([6, 5, 3], np.int32), np.array([3, 2, 1], np.int32)
    z, w, labels, tl, ll, mask = _problem("ag", "f32", N, T, U, A, blank, lengths=(tl, ll))
    z, w = torch.nan_to_num(z), torch.nan_to_num(w)
    lab, ttl, tll = dev(labels, tl, ll)
    zd = z.to(DEV).requires_grad_()
    teacher = w.to(DEV).requires_grad_()                        # (a teacher that requires grad gets None)
    loss = TransducerKDLoss(blank, mode, tau, reduction)(zd, teacher, lab, ttl, tll)
    go = torch.tensor([0.7, -1.3, 2.0][:loss.numel()], device=DEV).view(loss.shape)
    (loss * go).sum().backward()
    assert teacher.grad is None
    z64 = z.double().to(DEV).requires_grad_()
    want = kd_loss_torch(z64, w.double().to(DEV), lab, ttl, tll, blank, mode, tau, reduction)
    (want * go.double()).sum().backward()
    wts = np.broadcast_to(go.cpu().numpy().reshape(-1), (N,)) / (N if reduction == "mean" else 1)
    ref = Ref(z, w, labels, tl, ll, blank, F.MODES.index(mode), tau, weights=wts)
    tol = COST_TOL["f32"] * ref.cmag.sum() + COST_TOL["f32"]
    assert loss.shape == want.shape and (loss.double() - want).abs().max().item() <= tol
    ref.g = z64.grad.cpu().numpy()                              # the torch route's gradient, at the reference's bound
    check_grads("f32", zd.grad.double().cpu().numpy(), ref, what="%s %s" % (mode, reduction))


def test_gradcheck_fp64():
    from warprnnt_pytorch.kd import rnnt_kd_loss
    N, T, U, A, blank = 2, 4, 3, 5, 2
    rng = np.random.default_rng(2)
    lab, ttl, tll = dev(rng.integers(0, A, size=(N, U - 1)).astype(np.int32), np.array([4, 3], np.int32), np.array([2, 1], np.int32))
    w = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float64, device=DEV)
    for mode in ("collapsed", "full"):
        x = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float64, device=DEV, requires_grad=True)
        assert torch.autograd.gradcheck(lambda z: rnnt_kd_loss(z, w, lab, ttl, tll, blank, mode, 1.5, "none"), (x,), eps=1e-6,
                                        atol=1e-6, nondet_tol=1e-12)


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once on one stream (a linear chain), replayed twice on new logits."""
    from warprnnt_pytorch.kd import rnnt_kd_loss
    N, T, U, A, blank, tau = 3, 8, 5, 33, 32, 2.0
    rng = np.random.default_rng(11)
    tl, ll = np.array([8, 6, 4], np.int32), np.array([4, 0, 2], np.int32)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    lab, ttl, tll = dev(labels, tl, ll)
    static_z = torch.zeros((N, T, U, A), device=DEV, requires_grad=True)
    static_w = torch.zeros((N, T, U, A), device=DEV)
    k = _kd()
    k.lib()
    k.workspace_bytes(T, U, N, 0)

    def step():
        static_z.grad = None
        loss = rnnt_kd_loss(static_z, static_w, lab, ttl, tll, blank, "collapsed", tau, "sum", validate=False)
        loss.backward()
        return loss

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    static_z.grad = None
    with torch.cuda.graph(graph):
        loss = step()
    grad = static_z.grad
    for seed in (1, 2):
        r = np.random.default_rng(seed)
        zn, wn = (r.standard_normal((N, T, U, A)).astype(np.float32) * 2 for _ in range(2))
        with torch.no_grad():
            static_z.copy_(torch.tensor(zn))
            static_w.copy_(torch.tensor(wn))
        graph.replay()
        torch.cuda.synchronize()
        ref = Ref(torch.tensor(zn), torch.tensor(wn), labels, tl, ll, blank, 0, tau)
        assert abs(loss.item() - ref.c.sum()) <= COST_TOL["f32"] * ref.cmag.sum() + COST_TOL["f32"]
        check_grads("f32", grad.double().cpu().numpy(), ref, what="replay %d" % seed)


# ----------------------------------------------------------------------------- 64-bit addressing
def test_bf16_past_2_31_elements():
    """bf16, collapsed, N T U A = 3.5e9 elements, not a multiple of a packet (the stream's scalar tail writes the end of the
    tensor's last row).  The last sample is full, so the tensor's last row is inside a lattice; element 2^31 lies in sample
    3.  Gradients are compared with the reference on 300 rows: every in-lattice row of the four small samples -- the tensor's
    first row and the rows either side of element 2^31 among them -- and of the full sample its first row, the tensor's last
    row and random ones.  Costs are compared for the four small samples, all of whose rows are among the 300."""
    N, T, U, A, blank = 5, 63, 65, 171163, 70000
    TU = T * U
    E = N * TU * A
    at = 2 ** 31 // A                                            # the row that holds element 2^31
    assert E > 2 ** 31 and E % 8 != 0 and at == 3 * TU + 4 * U + 1 and at * A < 2 ** 31 < (at + 1) * A
    need = 3 * 2 * E + (1 << 30)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        print("SKIPPED: %d bytes of device memory free, three tensors past 2^31 elements need %d" % (free, need))
        pytest.skip("device memory is short")
    tl, ll = np.array([3, 1, 2, 6, T], np.int32), np.array([2, 3, 0, 3, U - 1], np.int32)
    mask = R.in_lattice_mask((N, T, U), tl, ll)
    assert mask.reshape(-1)[[0, at - 1, at, at + 1, N * TU - 1]].all()
    rng = np.random.default_rng(13)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    small = [tuple(r) for r in np.argwhere(mask[:4])]
    rows = small + [(4, 0, 0), (4, T - 1, U - 1)]
    rows += [(4, int(q) // U, int(q) % U) for q in rng.choice(np.arange(1, TU - 1), 300 - len(rows), replace=False)]
    rows = np.array(rows)
    assert len(rows) == 300 and len(small) == 39 and (0, 0, 0) in small and (3, 4, 1) in small
    gen = torch.Generator(device=DEV).manual_seed(1)
    z = torch.randn((N, T, U, A), generator=gen, device=DEV, dtype=torch.bfloat16)
    w = torch.randn((N, T, U, A), generator=gen, device=DEV, dtype=torch.bfloat16)
    g = torch.empty_like(z)
    st, c, _ = call(z, w, labels, tl, ll, blank, 0, 1.0, "score")
    assert st == 0
    k = _kd()
    lab, ttl, tll = dev(labels, tl, ll)
    ws = torch.empty(k.workspace_bytes(T, U, N, 2), dtype=torch.uint8, device=DEV)
    costs = torch.empty(N, device=DEV)
    st = k.lib().compute_kd_loss(z.data_ptr(), w.data_ptr(), g.data_ptr(), lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N,
                                 costs.data_ptr(), ws.data_ptr(), options(T, U, blank), 2, 0, ctypes.c_float(1.0))
    torch.cuda.synchronize()
    assert st == 0 and np.array_equal(costs.cpu().numpy(), c) and np.isfinite(c).all()
    zr, wr, gr = (torch.stack([x[b, t, u] for b, t, u in rows]).double().cpu().numpy() for x in (z, w, g))
    cl = R.class_labels(labels, ll, blank, A, U)
    kl, rg, cmag, gmag = R.kd_rows(zr, wr, np.array([cl[b, u] for b, _, u in rows]), blank, 1.0)
    for b in range(4):
        mine = rows[:, 0] == b
        bound = COST_TOL["bf16"] * cmag[mine].sum() + COST_TOL["bf16"]
        assert abs(c[b] - kl[mine].sum()) <= bound, (b, c[b], kl[mine].sum(), bound)
        assert g[b, tl[b]:].count_nonzero().item() == 0 and g[b, :tl[b], ll[b] + 1:].count_nonzero().item() == 0
    O.assert_grads(gr, rg, gmag, torch.bfloat16, what="300 rows of a tensor past 2^31 elements")
