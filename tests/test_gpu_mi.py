"""-m gpu: the lattice primitive on px / py edge log-probabilities (include/rnnt_mi.h, libwarprnnt_mi.so).

Every case of tests/mi_forms.py runs through the one-call C-ABI entry under torch.profiler with gradients: exactly the kernels
its release rules predict run, stage by stage.  Scores go against the fp64 reference of tests/mi_ref.py at COST_TOL (-inf
position for position), gradients per element at oracle.grad_bound(ref, |ref|, dtype), exact zeros outside every rectangle's
edges and for a sample without a path.  Inputs are NaN outside the rectangles' edge sets (never read), gradient buffers start
as NaN (every element is written).  The reference is given the stored values of the inputs.

A negative control compares the result with one boundary against the reference with another and must fail.  Then the
cross-checks against RNNTLoss and MonotonicRNNTLoss, the call forms, bit-identical reruns and workspaces, the edge cases of the
header, the invalid arguments and limits, autograd, a HIP-graph capture and two long lattices."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import mi_forms as F
from tests import mi_ref as R
from tests.gpu_support import CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, profiled, stages_seen
from tests.side_check import _BOUND_DTYPE

pytestmark = pytest.mark.gpu
NEG = float("-inf")


def _mi():
    from warprnnt_pytorch import mi
    return mi


def _opt(stream=None):
    return G.options(1, 1, 0, stream)                   # (only loc and stream are read)


def _problem(name, dtype, N, S, T, mod, bd=None, rng=None, poison_outside=True):
    """px, py of the storage type on the CPU: weights around -1.5, NaN outside every rectangle's edge sets; the boundary
    rows and the two edge masks."""
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    bd = R.full_boundary(N, S, T) if bd is None else np.asarray(bd, np.int64)
    px = torch.tensor(rng.standard_normal((N, S, T if mod else T + 1)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    mx, my = R.edge_masks(N, S, T, mod, bd)
    if poison_outside:
        px[torch.tensor(~mx)] = float("nan")
        py[torch.tensor(~my)] = float("nan")
    return px, py, bd, mx, my


def _table_problem(case, seed=None):
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()) if seed is None else seed)
    bd = F.boundaries(case, rng)
    return _problem(case["name"], case["dtype"], case["N"], case["S"], case["T"], case["mod"], bd, rng)


def call(px, py, bd=None, form="one", scale=None, gx=None, gy=None, ws=None, stream=None, prepare=None):
    """One C-ABI call form on device tensors -> (status, scores, px_grad, py_grad) as numpy (gradients float64, None where the
    form has none).  form: one | two | score | host, and the halves of `two` on the workspace `ws`, fwd | bwd.  Scores and
    gradients start as NaN."""
    m = _mi()
    N, S1, T = py.shape
    S, mod = S1 - 1, int(px.shape[2] == T)
    dtype = NAME[py.dtype]
    code = CODE[dtype]
    cdt = torch.float64 if dtype == "f64" else torch.float32
    lib = m.lib()
    bt = None if bd is None else torch.tensor(np.asarray(bd, np.int64), device=DEV)
    bp = None if bt is None else bt.data_ptr()
    xp = px.data_ptr() if px.numel() else None
    if ws is None:
        ws = torch.empty(m.workspace_bytes(S, T, N, mod, code), dtype=torch.uint8, device=DEV)
    scores = torch.full((N,), float("nan"), dtype=cdt, device=DEV)
    opt = _opt(stream)
    nograd = form in ("score", "fwd")
    if not nograd:
        gx = torch.full_like(px, float("nan")) if gx is None else gx
        gy = torch.full_like(py, float("nan")) if gy is None else gy
    gxp = None if nograd else (gx.data_ptr() if gx.numel() else None)
    gyp = None if nograd else gy.data_ptr()
    out = lambda t: None if t is None or nograd else t.double().cpu().numpy()     # noqa: E731
    if form == "host":
        hc = np.full(N, np.nan, dtype=np.float64 if dtype == "f64" else np.float32)
        st = lib.compute_rnnt_mi(xp, py.data_ptr(), bp, S, T, N, mod, hc.ctypes.data, gxp, gyp, ws.data_ptr(), opt, code)
        return st, hc, out(gx), out(gy)
    if form in ("one", "score"):
        st = lib.compute_rnnt_mi(xp, py.data_ptr(), bp, S, T, N, mod, scores.data_ptr(), gxp, gyp, ws.data_ptr(), opt, code)
    else:
        st = 0
        if form != "bwd":
            st = lib.compute_rnnt_mi_fwd(xp, py.data_ptr(), bp, S, T, N, mod, scores.data_ptr(), ws.data_ptr(), opt, code,
                                         1 if prepare is None else prepare)
            assert st == 0
    if form in ("two", "bwd"):
        sc = None if scale is None else torch.tensor(np.asarray(scale, np.float64), dtype=cdt, device=DEV)
        st = lib.compute_rnnt_mi_bwd(gxp, gyp, None if sc is None else sc.data_ptr(), S, T, N, mod, ws.data_ptr(), opt, code)
    torch.cuda.synchronize()
    return st, scores.cpu().numpy(), out(gx), out(gy)


def _reference(px, py, bd=None, weights=None):
    """The fp64 reference on the stored values (what lies outside the rectangles is never looked at: zeroed here)."""
    return R.mi_autograd(torch.nan_to_num(px.double().cpu(), nan=0.0, posinf=0.0, neginf=NEG).numpy(),
                         torch.nan_to_num(py.double().cpu(), nan=0.0, posinf=0.0, neginf=NEG).numpy(), bd, weights)


def _check(dtype, sc, gx, gy, rsc, rgx, rgy, mx, my, scale=None, what=""):
    """Scores at COST_TOL (-inf where the reference has it), gradients per element at oracle.grad_bound(ref, |ref|, dtype),
    exact zeros outside the rectangles' edges and for samples without a path.  gx None: scores only."""
    tol = COST_TOL[dtype]
    fin = np.isfinite(rsc)
    assert not np.isnan(rsc).any() and not np.isposinf(rsc).any(), (what, rsc)
    if fin.any():
        print(what, "max |dscore| = %.3e" % np.abs(sc[fin] - rsc[fin]).max())
    assert np.array_equal(np.isneginf(sc), np.isneginf(rsc)), (what, sc, rsc)
    assert np.allclose(sc[fin], rsc[fin], rtol=tol, atol=tol), (what, sc, rsc)
    if gx is None:
        return
    w = np.ones(len(rsc)) if scale is None else np.abs(np.asarray(scale, np.float64))
    worst = 0.0
    for got, ref, mask, nm in ((gx, rgx, mx, "px_grad"), (gy, rgy, my, "py_grad")):
        assert got.shape == ref.shape, (what, nm, got.shape, ref.shape)
        assert not got[~mask].any(), (what, nm, "exact zeros outside the rectangle's edges")          # (NaN counts as nonzero)
        for b in range(len(rsc)):
            if not fin[b]:
                assert not got[b].any(), (what, nm, b, "no path: zero gradients")
                continue
            m = mask[b]
            if not m.any():
                continue
            r = O.grad_check(got[b][m], ref[b][m], np.abs(ref[b][m]), _BOUND_DTYPE[dtype], scale=max(w[b], 1e-30))
            worst = max(worst, r["max_err_over_quantum"])
            assert r["passed"], ("%s %s sample %d" % (what, nm, b), r)
    print(what, "max gradient error / bound = %.3f" % worst)


# ----------------------------------------------------------------------------- every form of tests/mi_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_mi_form(name):
    case = F.CASES[name]
    px, py, bd, mx, my = _table_problem(case)
    xd, yd = px.to(DEV), py.to(DEV)
    run = lambda: call(xd, yd, bd, "one")                                                    # noqa: E731
    (st, sc, gx, gy), names = profiled(run)
    if st == 0 and not names:                        # (a profiler session now and then records no device event at all:
        (st, sc, gx, gy), names = profiled(run)      #  one more session, judged as the first would have been)
    assert st == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, G.cus()))
    rsc, rgx, rgy = _reference(px, py, bd)
    _check(case["dtype"], sc, gx, gy, rsc, rgx, rgy, mx, my, what=name)
    if case["N"] >= F.PATTERNS:
        assert np.isfinite(rsc[3]) and (case["mod"] or np.isfinite(rsc).all()), rsc
        if case["mod"] and case["S"] > 0:
            assert np.isneginf(rsc[6]) and np.isfinite(rsc[5]), rsc


def test_every_mi_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", False), ("f16", True)])
def test_negative_control_another_boundary_is_refused(dtype, mod):
    """The result with one boundary against the reference with another must fail, for the scores and for both gradients: the
    checks cannot pass on a library that ignores the boundary."""
    N, S, T = 4, 5, 9
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 8], [0, 1, 3, 9], [2, 0, 5, 7]], np.int64)
    other = np.array([[0, 1, 5, 9], [1, 2, 4, 7], [0, 1, 4, 9], [1, 0, 5, 7]], np.int64)
    px, py, bd, mx, my = _problem("neg", dtype, N, S, T, mod, bd, poison_outside=False)
    st, sc, gx, gy = call(px.to(DEV), py.to(DEV), bd, "one")
    assert st == 0
    rsc, rgx, rgy = _reference(px, py, bd)
    assert np.isfinite(rsc).all()
    _check(dtype, sc, gx, gy, rsc, rgx, rgy, mx, my, what="own boundary")
    osc, ogx, ogy = _reference(px, py, other)
    ox, oy = R.edge_masks(N, S, T, mod, other)
    assert (np.abs(osc - rsc) >= 100 * COST_TOL[dtype] * np.abs(rsc)).all(), (osc, rsc)      # (on the CPU: the references differ)
    with pytest.raises(AssertionError):
        _check(dtype, sc, None, None, osc, ogx, ogy, ox, oy, what="other scores")
    with pytest.raises(AssertionError):
        _check(dtype, osc, gx, ogy, osc, ogx, ogy, ox, oy, what="other px_grad")
    with pytest.raises(AssertionError):
        _check(dtype, osc, ogx, gy, osc, ogx, ogy, ox, oy, what="other py_grad")


# ----------------------------------------------------------------------------- against the losses of this tree, fp64
def _from_logits(x, labels, tl, ll, blank, mod):
    """px, py (fp64, on the device) gathered from log_softmax(x), x (N, T, U, A); the regular type's column T_b at -inf; the
    boundary rows [0, 0, L_b, T_b]."""
    N, T, U, A = x.shape
    lsm = torch.log_softmax(x, -1)
    py = lsm[..., blank].transpose(1, 2).contiguous()                                        # (N, U, T)
    idx = torch.tensor(labels, device=x.device, dtype=torch.int64)[:, None, :, None].expand(N, T, U - 1, 1)
    lab = lsm[:, :, :U - 1].gather(3, idx)[..., 0].transpose(1, 2)                           # (N, U - 1, T)
    if mod:
        px = lab.contiguous()
    else:
        px = torch.cat((lab, torch.full((N, U - 1, 1), NEG, dtype=x.dtype, device=x.device)), 2)
        for b in range(N):
            px[b, :, int(tl[b])] = NEG
        px = px.contiguous()
    bd = np.stack((np.zeros(N), np.zeros(N), ll, tl), 1).astype(np.int64)
    return px, py, bd


def _coefficients(grad, x, labels, blank):
    """(cb, cl) (N, T, U) implied by d cost / d logits = (cb + cl) softmax - [blank] cb - [label] cl: cb + cl from the columns
    that are neither (their gradient and softmax summed), then each from its own column."""
    N, T, U, A = x.shape
    sm = torch.softmax(x, -1)
    other = torch.ones((N, T, U, A), dtype=torch.bool, device=x.device)
    other[..., blank] = False
    lab = torch.tensor(labels, device=x.device, dtype=torch.int64)
    lab = torch.cat((lab, torch.full((N, 1), blank, device=x.device, dtype=torch.int64)), 1)[:, None, :, None].expand(N, T, U, 1)
    other.scatter_(3, lab, False)
    tot = (grad * other).sum(-1) / (sm * other).sum(-1)
    cb = tot * sm[..., blank] - grad[..., blank]
    cl = tot * sm.gather(3, lab)[..., 0] - grad.gather(3, lab)[..., 0]
    return cb, cl


@pytest.mark.parametrize("mod", [False, True])
def test_scores_and_occupations_are_the_losses_of_this_tree(mod):
    """scores == -RNNTLoss(x) (regular) / -MonotonicRNNTLoss(x) (modified) at rtol = 1e-9, fp64, and the occupations are the
    blank / label coefficients those losses' gradients imply."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.mi import mutual_information_recursion
    from warprnnt_pytorch.mono import MonotonicRNNTLoss
    N, T, U, A, blank = 4, 12, 5, 37, 9
    rng = np.random.default_rng(17)
    tl, ll = np.array([12, 5 if mod else 1, 7, 9], np.int32), np.array([4, 2, 0, 3], np.int32)
    labels = rng.choice([c for c in range(A) if c != blank], size=(N, U - 1)).astype(np.int32)
    x = torch.tensor(rng.standard_normal((N, T, U, A)) * 2, dtype=torch.float64, device=DEV)
    lab, ttl, tll = G.dev(labels, tl, ll)
    xa = x.clone().requires_grad_()
    loss = (MonotonicRNNTLoss if mod else RNNTLoss)(blank=blank, reduction="none")(xa, lab, ttl, tll)
    loss.sum().backward()
    px, py, bd = _from_logits(x, labels, tl, ll, blank, mod)
    scores, (gx, gy) = mutual_information_recursion(px, py, torch.tensor(bd, device=DEV), return_grad=True)
    assert torch.allclose(scores, -loss.detach(), rtol=1e-9, atol=0), (scores, loss)
    cb, cl = _coefficients(xa.grad, x, labels, blank)
    mx, my = R.edge_masks(N, U - 1, T, mod, bd)
    want_y = cb.transpose(1, 2).cpu().numpy()                                                # (N, U, T)
    want_x = cl[:, :, :U - 1].transpose(1, 2).cpu().numpy()                                  # (N, U - 1, T)
    gx, gy = gx.cpu().numpy(), gy.cpu().numpy()
    assert not gx[~mx].any() and not gy[~my].any()
    if not mod:
        assert not gx[:, :, T].any()                                                         # (the -inf column)
        gx, mx = gx[:, :, :T], mx[:, :, :T]
    O.assert_grads(gy[my], want_y[my], np.abs(want_y[my]), torch.float64, what="py_grad == cb")
    O.assert_grads(gx[mx], want_x[mx], np.abs(want_x[mx]), torch.float64, what="px_grad == cl")


# ----------------------------------------------------------------------------- call forms and workspaces
@pytest.mark.parametrize("dtype,S,mod", [("f32", 8, False), ("bf16", 8, True), ("f32", 65, True), ("f64", 69, False)])
def test_call_forms_agree(dtype, S, mod):
    N, T = 7, 75 if mod else 11
    case = dict(name="forms_%s_%d" % (dtype, S), dtype=dtype, N=N, S=S, T=T, mod=mod)
    px, py, bd, mx, my = _table_problem(case, seed=S)
    xd, yd = px.to(DEV), py.to(DEV)
    for bdx in (bd, None):
        if bdx is None:                              # the full rectangles read everything: no NaN
            px, py, _, mx, my = _problem("full", dtype, N, S, T, mod, None, np.random.default_rng(S))
            xd, yd = px.to(DEV), py.to(DEV)
        st, s1, gx1, gy1 = call(xd, yd, bdx, "one")
        assert st == 0
        rsc, rgx, rgy = _reference(px, py, bdx)
        _check(dtype, s1, gx1, gy1, rsc, rgx, rgy, mx, my, what="one call")
        st, s2, gx2, gy2 = call(xd, yd, bdx, "two", scale=np.ones(N))
        assert st == 0 and np.array_equal(s1, s2, equal_nan=True) and np.array_equal(gx1, gx2) and np.array_equal(gy1, gy2)
        st, s2, gx2, gy2 = call(xd, yd, bdx, "two")                                          # (a NULL scale)
        assert st == 0 and np.array_equal(s1, s2) and np.array_equal(gx1, gx2) and np.array_equal(gy1, gy2)
        (st, s3, _, _), names = profiled(lambda: call(xd, yd, bdx, "score"))
        assert st == 0 and np.array_equal(s1, s3)
        seen = stages_seen(names, F.stage_of, F.STAGES)
        want = F.predict(case, G.cus())
        assert not names or (seen["pack"] == want["pack"] and seen["lattice"] == want["lattice"] and not seen["unpack"]), seen
        st, s4, gx4, gy4 = call(xd, yd, bdx, "host")
        assert st == 0 and np.array_equal(s1.astype(s4.dtype), s4) and np.array_equal(gx1, gx4) and np.array_equal(gy1, gy4)
        scale = 0.5 + 0.25 * np.arange(N)
        scale[1] = -1.5
        st, s6, gx6, gy6 = call(xd, yd, bdx, "two", scale=scale)
        assert st == 0 and np.array_equal(s1, s6)
        wsc, wgx, wgy = _reference(px, py, bdx, weights=scale)
        _check(dtype, s6, gx6, gy6, wsc, wgx, wgy, mx, my, scale=scale, what="two-phase, weighted")
        st, s7, gx7, gy7 = call(xd, yd, bdx, "one")                                          # a second run: identical bits
        assert st == 0 and np.array_equal(s1, s7) and np.array_equal(gx1, gx7) and np.array_equal(gy1, gy7)


@pytest.mark.parametrize("S,mod", [(6, False), (6, True), (70, False), (70, True)])
def test_workspace_contents_do_not_matter(S, mod):
    """A workspace full of 0xFF bytes (NaN as values, -1 as flags and lengths) gives the bits a zeroed one gives."""
    m = _mi()
    N, T = 7, 80 if mod else 13
    case = dict(name="ws", dtype="f32", N=N, S=S, T=T, mod=mod)
    px, py, bd, mx, my = _table_problem(case, seed=S)
    xd, yd = px.to(DEV), py.to(DEV)
    out = []
    for fill in (0, 255):
        ws = torch.full((m.workspace_bytes(S, T, N, int(mod), 0),), fill, dtype=torch.uint8, device=DEV)
        st, sc, gx, gy = call(xd, yd, bd, "one", ws=ws)
        assert st == 0
        out.append((sc, gx, gy))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    rsc, rgx, rgy = _reference(px, py, bd)
    _check("f32", *out[1], rsc, rgx, rgy, mx, my, what="0xFF workspace")


# ----------------------------------------------------------------------------- the header's edge cases
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("mod", [False, True])
def test_infinite_and_non_finite_edges(dtype, mod):
    """-inf edges with a path left: a limit; no path: -inf and zero gradients; NaN / +inf on an edge of the rectangle: that
    sample only -- NaN score, NaN on the rectangle's edges, zeros outside; a NaN outside every rectangle changes nothing."""
    N, S, T = 8, 4, 7
    bd = R.full_boundary(N, S, T)
    bd[3] = (1, 1, 3, 6)
    bd[6] = (0, 2, 4, 7)
    px, py, bd, mx, my = _problem("nf", dtype, N, S, T, mod, bd, poison_outside=False)
    inf = float("inf")
    px[0, 1, 2] = NEG                                   # holes with paths around them
    py[0, 2, 3] = NEG
    py[0, 0, 0] = NEG
    if not mod:
        px[0, :, T] = NEG                               # k2's own -inf column
    px[1, 2, :] = NEG                                   # symbol 2 can never be emitted: no path
    py[2, :, T - 1] = NEG if mod else py[2, :, T - 1]   # modified: the last frame closed but for the symbol edges
    px[2, :, T - 1] = NEG if mod else px[2, :, T - 1]   #           ... and those too: no path
    px[3, 1, 3] = float("nan")                          # inside sample 3's rectangle
    py[4, 4, 6] = inf
    px[5, 0, 0] = inf
    py[6, 0, 0] = float("nan")                          # outside sample 6's rectangle (t0 = 2): nothing changes
    px[6, 3, 1] = inf
    st, sc, gx, gy = call(px.to(DEV), py.to(DEV), bd, "one")
    assert st == 0
    for b in (3, 4, 5):
        assert np.isnan(sc[b]), (b, sc)
        assert np.isnan(gx[b][mx[b]]).all() and np.isnan(gy[b][my[b]]).all(), b
        assert not gx[b][~mx[b]].any() and not gy[b][~my[b]].any(), b
    keep = [0, 1, 2, 6, 7]
    rsc, rgx, rgy = _reference(px[keep], py[keep], bd[keep])
    assert np.isfinite(rsc[0]) and np.isneginf(rsc[1]) and np.isneginf(rsc[2]) == mod and np.isfinite(rsc[3:]).all(), rsc
    _check(dtype, sc[keep], gx[keep], gy[keep], rsc, rgx, rgy, mx[keep], my[keep], what="limits")


@pytest.mark.parametrize("mod", [False, True])
def test_degenerate_rectangles_closed_forms(mod):
    """fp64.  s1 == s0: the frames alone, sum of py; t1 == t0: regular sum of px[., t0], modified 0 when s1 == s0 and -inf
    otherwise; S = 0: px has no element; modified with s1 - s0 == t1 - t0: the diagonal of px."""
    N, S, T = 5, 3, 6
    bd = np.array([[2, 1, 2, 5], [0, 4, 3, 4], [1, 3, 1, 3], [0, 2, 3, 5], [0, 0, 3, 6]], np.int64)
    px, py, bd, mx, my = _problem("deg", "f64", N, S, T, mod, bd)
    st, sc, gx, gy = call(px.to(DEV), py.to(DEV), bd, "one")
    assert st == 0
    X, Y = px.numpy(), py.numpy()
    assert not gx[~mx].any() and not gy[~my].any()
    one = lambda v, n: v.shape == (n,) and np.allclose(v, 1.0, rtol=1e-12, atol=0)           # noqa: E731
    assert abs(sc[0] - Y[0, 2, 1:5].sum()) < 1e-12 and not gx[0].any() and one(gy[0][my[0]], 4)
    if mod:
        assert np.isneginf(sc[1]) and sc[2] == 0 and not gx[1].any() and not gy[1].any()
        assert abs(sc[3] - sum(X[3, i, 2 + i] for i in range(3))) < 1e-12 and abs(gx[3].sum() - 3) < 1e-12 and not gy[3].any()
    else:
        assert abs(sc[1] - X[1, :, 4].sum()) < 1e-12 and one(gx[1][mx[1]], 3) and not gy[1].any() and sc[2] == 0
    assert not gx[2].any() and not gy[2].any()
    # S = 0
    px0, py0, bd0, mx0, my0 = _problem("s0", "f64", 3, 0, 9, mod, np.array([[0, 0, 0, 9], [0, 3, 0, 4], [0, 5, 0, 5]]))
    for form in ("one", "two", "host"):
        st, sc, gx, gy = call(px0.to(DEV), py0.to(DEV), bd0, form)
        Y = py0.numpy()
        assert st == 0 and gx.size == 0 and np.allclose(sc, [Y[0, 0].sum(), Y[1, 0, 3], 0.0], rtol=1e-12, atol=0)
        assert not gy[~my0].any() and one(gy[my0], 9 + 1 + 0)


def test_invalid_arguments():
    m = _mi()
    lib = m.lib()
    N, S, T = 3, 4, 6
    px, py, bd, mx, my = _problem("inv", "f32", N, S, T, False, poison_outside=False)
    xd, yd = px.to(DEV), py.to(DEV)
    st, sc, gx, gy = call(xd, yd, None, "one")
    assert st == 0 and np.isfinite(sc).all()
    # a boundary outside the tensor: the marker -> INVALID_VALUE with host scores; enqueue-only forms mark the sample alone
    for row in ((0, 0, S + 1, T), (0, 0, S, T + 1), (-1, 0, S, T), (0, -1, S, T), (3, 0, 2, T), (0, 5, S, 4),
                (0, 0, 2 ** 40, T), (-2 ** 62, 0, S, T)):
        bad = R.full_boundary(N, S, T)
        bad[1] = row
        for mod in (False, True):
            x2 = xd[:, :, :T].contiguous() if mod else xd
            st, _, _, _ = call(x2, yd, bad, "host")
            assert st == 2, row
            st, sc2, gx2, gy2 = call(x2, yd, bad, "one")
            assert st == 0 and np.isnan(sc2[1]) and np.isfinite(sc2[[0, 2]]).all(), (row, sc2)
            assert sc2[1:2].view(np.uint32)[0] == 0x7fc0dead
            assert not gx2[1].any() and not gy2[1].any() and gx2[0].any() and gy2[2].any()
            if not mod:
                assert np.array_equal(sc2[[0, 2]], sc[[0, 2]]) and np.array_equal(gx2[0], gx[0]) and np.array_equal(gy2[2], gy[2])
    # one gradient without the other; NULL pointers; dtype codes; the CPU location
    ws = torch.empty(m.workspace_bytes(S, T, N, 0, 1), dtype=torch.uint8, device=DEV)
    scores = torch.zeros(N, device=DEV)
    gxt, gyt = torch.zeros_like(xd), torch.zeros_like(yd)
    one = lambda **kw: lib.compute_rnnt_mi(                                                              # noqa: E731
        kw.get("px", xd.data_ptr()), kw.get("py", yd.data_ptr()), None, kw.get("S", S), kw.get("T", T), kw.get("N", N), 0,
        kw.get("scores", scores.data_ptr()), kw.get("gx", gxt.data_ptr()), kw.get("gy", gyt.data_ptr()),
        kw.get("ws", ws.data_ptr()), kw.get("opt", _opt()), kw.get("code", 0))
    assert one() == 0 and one(gx=None, gy=None) == 0
    assert one(gx=None) == 2 and one(gy=None) == 2
    assert one(px=None) == 2 and one(py=None) == 2 and one(scores=None) == 2 and one(ws=None) == 2
    for code in (4, -1):
        assert one(code=code) == 2
    cpu = _opt()
    cpu.loc = 0
    assert one(opt=cpu) == 2
    assert one(S=-1) == 2 and one(T=0) == 2 and one(N=0) == 2
    # overlaps: a gradient inside an input, the other gradient or the workspace; off its element boundary
    assert one(gx=yd.data_ptr()) == 2 and one(gy=xd.data_ptr() + 16) == 2 and one(gx=xd.data_ptr()) == 2
    assert one(gx=gyt.data_ptr() + 8) == 2 and one(gy=ws.data_ptr() + 256) == 2 and one(gx=gxt.data_ptr() + 2) == 2
    # the limits, before anything is touched
    assert one(S=4096) == 2 and one(S=4095, T=(1 << 13) - 1) == 2 and one(S=15, T=(1 << 12) - 1, N=1 << 16) == 2
    n = C.c_size_t(0)
    assert lib.get_workspace_size_mi(4, 3, 1, 0, 4, C.byref(n)) == 2 and lib.get_workspace_size_mi(4, 0, 1, 0, 0, C.byref(n)) == 2
    assert lib.get_workspace_size_mi(4, 3, 1, 0, 0, None) == 2
    assert lib.get_workspace_size_mi(4, 3, 1, 0, 0, C.byref(n)) == 0 and n.value > 0
    assert lib.compute_rnnt_mi_bwd(None, gyt.data_ptr(), None, S, T, N, 0, ws.data_ptr(), _opt(), 0) == 2
    assert lib.compute_rnnt_mi_bwd(gxt.data_ptr(), None, None, S, T, N, 0, ws.data_ptr(), _opt(), 0) == 2
    assert lib.compute_rnnt_mi_fwd(xd.data_ptr(), yd.data_ptr(), None, S, T, N, 0, None, ws.data_ptr(), _opt(), 0, 1) == 2
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the Python module
def test_python_validation_on_the_device():
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    px, py = torch.zeros(2, 3, 6, device=DEV), torch.zeros(2, 4, 5, device=DEV)
    for row in ((0, 0, 4, 5), (0, 0, 3, 6), (2, 0, 1, 5), (0, -1, 3, 5)):
        bd = torch.tensor([[0, 0, 3, 5], row], device=DEV)
        with pytest.raises(ValueError, match="boundary\\[1\\]"):
            mir(px, py, bd)
        sc = mir(px, py, bd, validate=False)          # enqueue only: the library marks the sample
        assert torch.isnan(sc[1]) and torch.isfinite(sc[0])
    with pytest.raises(ValueError, match="one device"):
        mir(px, py, torch.tensor([[0, 0, 3, 5]] * 2))
    with pytest.raises(ValueError, match="GPU only"):
        mir(px.cpu(), py)
    with pytest.raises(ValueError, match="px must be"):
        mir(torch.zeros(2, 3, 7, device=DEV), py)
    sc = mir(px, py)
    assert sc.dtype == torch.float32 and sc.shape == (2,)
    assert mir(px.bfloat16(), py.bfloat16()).dtype == torch.float32 and mir(px.double(), py.double()).dtype == torch.float64


@pytest.mark.parametrize("mod", [False, True])
def test_gradcheck_fp64(mod):
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    rng = np.random.default_rng(2)
    B, S, T = 3, 2, 4
    px = torch.tensor(rng.standard_normal((B, S, T if mod else T + 1)) - 1, dtype=torch.float64, device=DEV, requires_grad=True)
    py = torch.tensor(rng.standard_normal((B, S + 1, T)) - 1, dtype=torch.float64, device=DEV, requires_grad=True)
    bd = torch.tensor([[0, 0, 2, 4], [1, 1, 2, 4], [0, 0, 2, 3]], device=DEV)
    assert torch.autograd.gradcheck(lambda a, b: mir(a, b, bd), (px, py), eps=1e-6, atol=1e-6, nondet_tol=1e-12)
    assert torch.autograd.gradcheck(lambda a, b: mir(a, b, bd, return_grad=True)[0], (px, py), eps=1e-6, atol=1e-6,
                                    nondet_tol=1e-12)


@pytest.mark.parametrize("mod", [False, True])
def test_return_grad_and_requires_grad_combinations(mod):
    """return_grad with and without inputs that require grad, and requires grad without return_grad: the same scores bit for
    bit, the occupations of the reference, and backward = occupations times grad_output."""
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    case = dict(name="rg", dtype="f32", N=7, S=9, T=14, mod=mod)
    px, py, bd, mx, my = _table_problem(case, seed=3)
    xd, yd, bt = px.to(DEV), py.to(DEV), torch.tensor(bd, device=DEV)
    rsc, rgx, rgy = _reference(px, py, bd)
    go = torch.tensor([0.7, -1.3, 2.0, 1.0, 0.25, 3.0, -0.5], device=DEV)
    w = go.cpu().numpy().astype(np.float64)
    # 1: return_grad, nothing requires grad
    s1, (gx1, gy1) = mir(xd, yd, bt, return_grad=True)
    assert not s1.requires_grad and not gx1.requires_grad and gx1.shape == xd.shape and gy1.dtype == yd.dtype
    _check("f32", s1.cpu().numpy(), gx1.double().cpu().numpy(), gy1.double().cpu().numpy(), rsc, rgx, rgy, mx, my, what="1")
    # 2: return_grad and requires grad: one forward pass, backward multiplies
    xa, ya = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    (s2, (gx2, gy2)), names = profiled(lambda: mir(xa, ya, bt, return_grad=True))
    assert s2.requires_grad and not gx2.requires_grad and torch.equal(s2.detach(), s1)
    assert torch.equal(gx2, gx1) and torch.equal(gy2, gy1)
    assert sum(F.stage_of(n) == "unpack" for n in names) <= 1
    _, names = profiled(lambda: torch.where(torch.isfinite(s2), s2, torch.zeros_like(s2)).mul(go).sum().backward())
    assert not any(F.stage_of(n) is not None for n in names), names          # no kernel of the library in backward
    fin = torch.isfinite(s1).cpu().numpy()
    w2 = np.where(fin, w, 0.0)
    _, vgx, vgy = _reference(px, py, bd, weights=w2)
    _check("f32", s1.cpu().numpy(), xa.grad.double().cpu().numpy(), ya.grad.double().cpu().numpy(), rsc, vgx, vgy, mx, my,
           scale=np.where(fin, np.abs(w), 1.0), what="2")
    # 3: requires grad alone: two-phase, the scale inside the kernel
    xb, yb = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    s3 = mir(xb, yb, bt)
    assert torch.equal(s3.detach(), s1)
    torch.where(torch.isfinite(s3), s3, torch.zeros_like(s3)).mul(go).sum().backward()
    _check("f32", s1.cpu().numpy(), xb.grad.double().cpu().numpy(), yb.grad.double().cpu().numpy(), rsc, vgx, vgy, mx, my,
           scale=np.where(fin, np.abs(w), 1.0), what="3")


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch), replayed twice on new inputs."""
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    B, S, T = 3, 5, 9
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 9], [0, 0, 3, 6]], np.int64)
    bt = torch.tensor(bd, device=DEV)
    sx = torch.zeros((B, S, T + 1), device=DEV, requires_grad=True)
    sy = torch.zeros((B, S + 1, T), device=DEV, requires_grad=True)
    m = _mi()
    m.lib()
    m.workspace_bytes(S, T, B, False, 0)

    def step():
        sx.grad = sy.grad = None
        total = mir(sx, sy, bt, validate=False).sum()
        total.backward()
        return total

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    sx.grad = sy.grad = None
    with torch.cuda.graph(graph):
        total = mir(sx, sy, bt, validate=False).sum()
        total.backward()
    gxs, gys = sx.grad, sy.grad
    mx, my = R.edge_masks(B, S, T, False, bd)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        xn = (rng.standard_normal((B, S, T + 1)) - 1).astype(np.float32)
        yn = (rng.standard_normal((B, S + 1, T)) - 1).astype(np.float32)
        with torch.no_grad():
            sx.copy_(torch.tensor(xn))
            sy.copy_(torch.tensor(yn))
        graph.replay()
        torch.cuda.synchronize()
        rsc, rgx, rgy = R.mi_autograd(xn, yn, bd)
        assert abs(total.item() - rsc.sum()) < 1e-5 * abs(rsc.sum())
        _check("f32", rsc.astype(np.float32), gxs.double().cpu().numpy(), gys.double().cpu().numpy(), rsc, rgx, rgy, mx, my,
               what="replay %d" % seed)


# ----------------------------------------------------------------------------- long lattices: the offsets
@pytest.mark.parametrize("S", [300, 32])
def test_long_lattice(S):
    """T = 1500, fp32: the block form's per-diagonal offsets (S = 300, the second sample a short rectangle inside) and the wave
    form's per-chunk ones (S = 32, some 190 re-centrings)."""
    N, T = 2, 1500
    bd = np.array([[0, 0, S, T], [3, 40, min(S, 33), 140]], np.int64)
    px, py, bd, mx, my = _problem("long", "f32", N, S, T, False, bd)
    st, sc, gx, gy = call(px.to(DEV), py.to(DEV), bd, "one")
    assert st == 0
    rsc, rgx, rgy = _reference(px, py, bd)
    assert np.isfinite(rsc).all()
    _check("f32", sc, gx, gy, rsc, rgx, rgy, mx, my, what="long S = %d" % S)
