"""-m gpu: the expected path cost over px / py edge log-probabilities (include/rnnt_expect.h, libwarprnnt_expect.so).

Every case of tests/expect_forms.py runs through compute_rnnt_expect under torch.profiler with all outputs taken: exactly
the kernels its release rule predicts run, stage by stage.  Inputs are NaN outside the rectangles' edge sets (never read);
outputs start as NaN between 4096 guard bytes that stay as they were.  The reference (tests/expect_ref.py, numpy fp64) is given
the stored values.  The bounds follow from fp64 arithmetic on stored values; none is measured:

    scores              COST_TOL["f64"] = 1e-9 rtol / atol for every storage type, -inf and NaN position for position
    expect              |got - ref| <= 1e-9 (1 + Eabs[b]),                 Eabs the expected |cost|
    nodes               a as scores; A: |got - ref| <= 1e-9 (1 + the node's expected prefix |cost|); -inf position for position
    cx_grad, cy_grad    oracle.grad_check(got, ref, |ref|, dtype)
    px_grad, py_grad    oracle.grad_check(got, ref, mag, dtype), mag = |g_expect| occ_e (E[|C| | e] + Eabs[b]) + |g_score| occ_e

and exact zeros outside the rectangles' edges and for samples without a path.

Then: a negative control (another boundary), the call forms, reruns, the header's edge cases, limits and refusals, `mi` of this
tree as a yardstick, the Python module with gradcheck and a HIP-graph capture, a large batch and two long lattices."""
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import expect_forms as F
from tests import expect_ref as R
from tests import gpu_support as G
from tests.gpu_support import CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, profiled, stages_seen
from tests.side_check import _BOUND_DTYPE
from tests.test_gpu_bestpath import Guarded

pytestmark = pytest.mark.gpu
NEG = float("-inf")
TOL = COST_TOL["f64"]
GRADS = ("gx", "gy", "hx", "hy")
MARKER_BITS = 0x7ff8dead00000000


def _ex():
    from warprnnt_pytorch import expect
    return expect


def _opt(stream=None):
    return G.options(1, 1, 0, stream)                   # (only loc and stream are read)


def _problem(name, dtype, N, S, T, mod, bd=None, rng=None, poison_outside=True):
    """px, py, cx, cy of the storage type on the CPU: weights around -1.5, costs around 0, NaN outside every rectangle's edge
    sets; the boundary rows and the two edge masks."""
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    bd = R.full_boundary(N, S, T) if bd is None else np.asarray(bd, np.int64)
    xs, ys = (N, S, T if mod else T + 1), (N, S + 1, T)
    px = torch.tensor(rng.standard_normal(xs) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    py = torch.tensor(rng.standard_normal(ys) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    cx = torch.tensor(rng.standard_normal(xs) + 0.25, dtype=torch.float32).to(TORCH[dtype])
    cy = torch.tensor(rng.standard_normal(ys) - 0.25, dtype=torch.float32).to(TORCH[dtype])
    mx, my = R.edge_masks(N, S, T, mod, bd)
    if poison_outside:
        for t, m in ((px, mx), (cx, mx), (py, my), (cy, my)):
            t[torch.tensor(~m)] = float("nan")
    return px, py, cx, cy, bd, mx, my


def _table_problem(case, seed=None):
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()) if seed is None else seed)
    bd = F.boundaries(case, rng)
    return _problem(case["name"], case["dtype"], case["N"], case["S"], case["T"], case["mod"], bd, rng)


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def call(px, py, cx, cy, bd=None, form="all", ge=None, gs=None, stream=None):
    """One C-ABI call (or the two-phase pair) on device tensors -> dict(st, scores, expect, nodes, gx, gy, hx, hy) as numpy
    float64 (None where the form has none).  form: all (device scalars, four gradients) | nocost (px_grad / py_grad only) |
    fwdonly | host (host scalars, four gradients) | two (the _fwd and _bwd entries, scales ge / gs) | two_nocost.  Every output
    starts as NaN between guards."""
    lib = _ex().lib()
    N, S1, T = py.shape
    S, mod = S1 - 1, int(px.shape[2] == T)
    code = CODE[NAME[py.dtype]]
    bt = None if bd is None else torch.tensor(np.asarray(bd, np.int64), device=DEV)
    bp = None if bt is None else bt.data_ptr()
    p = lambda t: t.data_ptr() if t.numel() else None                                        # noqa: E731
    opt = _opt(stream)
    nan = float("nan")
    gsc, gex = Guarded((N,), torch.float64, nan), Guarded((N,), torch.float64, nan)
    gnd = Guarded((N, S + 1, T + 1, 2), torch.float64, nan)
    gr = {"gx": Guarded(tuple(px.shape), px.dtype, nan), "gy": Guarded(tuple(py.shape), py.dtype, nan),
          "hx": Guarded(tuple(px.shape), px.dtype, nan), "hy": Guarded(tuple(py.shape), py.dtype, nan)}
    taken = {"all": GRADS, "host": GRADS, "two": GRADS, "nocost": GRADS[:2], "two_nocost": GRADS[:2], "fwdonly": ()}[form]
    ptr = {k: (gr[k].ptr if k in taken else None) for k in GRADS}
    hs = he = None
    if form.startswith("two"):
        st = lib.compute_rnnt_expect_fwd(p(px), py.data_ptr(), p(cx), cy.data_ptr(), bp, S, T, N, mod, gsc.ptr, gex.ptr, gnd.ptr,
                                         opt, code)
        assert st == 0
        tge = None if ge is None else torch.tensor(np.asarray(ge, np.float64), device=DEV)
        tgs = None if gs is None else torch.tensor(np.asarray(gs, np.float64), device=DEV)
        st = lib.compute_rnnt_expect_bwd(p(px), py.data_ptr(), p(cx), cy.data_ptr(), bp, gnd.ptr, gsc.ptr, gex.ptr,
                                         None if tge is None else tge.data_ptr(), None if tgs is None else tgs.data_ptr(),
                                         S, T, N, mod, ptr["gx"], ptr["gy"], ptr["hx"], ptr["hy"], opt, code)
    else:
        if form == "host":
            hs, he = np.full(N, np.nan), np.full(N, np.nan)
        st = lib.compute_rnnt_expect(p(px), py.data_ptr(), p(cx), cy.data_ptr(), bp, S, T, N, mod,
                                     hs.ctypes.data if form == "host" else gsc.ptr, he.ctypes.data if form == "host" else gex.ptr,
                                     gnd.ptr, ptr["gx"], ptr["gy"], ptr["hx"], ptr["hy"], opt, code)
    torch.cuda.synchronize()
    for g in [gsc, gex, gnd] + list(gr.values()):
        assert g.guards_intact()
    out = dict(st=st, scores=hs if form == "host" else gsc.t.cpu().numpy(), expect=he if form == "host" else gex.t.cpu().numpy(),
               nodes=gnd.t.cpu().numpy())
    if form == "host":
        assert torch.isnan(gsc.t).all() and torch.isnan(gex.t).all()
    for k in GRADS:
        if k in taken:
            out[k] = gr[k].t.double().cpu().numpy()
        else:
            assert torch.isnan(gr[k].t).all()                                                # not taken: not touched
            out[k] = None
    return out


def _stored(t):
    return t.double().cpu().numpy()


def _reference(px, py, cx, cy, bd, mod, ge=None, gs=None):
    return R.expected_cost(_stored(px), _stored(py), _stored(cx), _stored(cy), bd, mod, ge, gs)


def _check(got, ref, dtype, mx, my, ge=None, gs=None, what=""):
    """Everything a call returned against the reference, at the bounds of the module's docstring.  -> the worst error over
    its bound."""
    N = len(ref["scores"])
    ge = np.ones(N) if ge is None else np.asarray(ge, np.float64)
    gs = np.zeros(N) if gs is None else np.asarray(gs, np.float64)
    worst = 0.0
    rs, re_ = ref["scores"], ref["expect"]
    fin = np.isfinite(rs)
    assert np.array_equal(got["scores"][~fin], rs[~fin], equal_nan=True), (what, "scores", got["scores"], rs)
    err = np.abs(got["scores"][fin] - rs[fin])
    bound = TOL + TOL * np.abs(rs[fin])
    assert (err <= bound).all(), (what, "scores", got["scores"], rs)
    worst = max(worst, float((err / bound).max()) if fin.any() else 0.0)
    efin = np.isfinite(re_)
    assert np.array_equal(np.isnan(got["expect"]), np.isnan(re_)), (what, "expect", got["expect"], re_)
    err = np.abs(got["expect"][efin] - re_[efin])
    bound = TOL * (1 + ref["Eabs"][efin])
    assert (err <= bound).all(), (what, "expect", got["expect"], re_, bound)
    worst = max(worst, float((err / bound).max()) if efin.any() else 0.0)
    for b in range(N):
        if not efin[b] and not (np.isnan(rs[b]) and rs[b:b + 1].view(np.uint64)[0] == MARKER_BITS):
            continue                                     # NaN weights or costs: the nodes are unspecified
        ga, gA, ra, rA = got["nodes"][b, ..., 0], got["nodes"][b, ..., 1], ref["nodes"][b, ..., 0], ref["nodes"][b, ..., 1]
        inf = np.isneginf(ra)
        assert np.array_equal(np.isneginf(ga), inf), (what, b, "nodes: -inf")
        ea, eA = np.abs(ga[~inf] - ra[~inf]), np.abs(gA - rA)
        ba, bA = TOL + TOL * np.abs(ra[~inf]), TOL * (1 + ref["nodes_abs"][b])
        assert (ea <= ba).all() and (eA <= bA).all(), (what, b, "nodes", float(ea.max(initial=0)), float(eA.max()))
        assert not gA[inf].any(), (what, b, "nodes: A of an unreachable node")
        worst = max(worst, float((ea / ba).max(initial=0)), float((eA / bA).max()))
    if got["gx"] is None:
        return worst
    name = _BOUND_DTYPE[dtype]
    for k, m in (("gx", mx), ("gy", my), ("hx", mx), ("hy", my)):
        if got[k] is None:
            continue
        g, r = got[k], ref[k]
        assert not g[~m].any(), (what, k, "nonzero outside the rectangles' edges")
        for b in range(N):
            if np.isnan(rs[b]) or np.isnan(re_[b]):      # NaN weights: NaN on the edges; NaN costs: unspecified
                if np.isnan(rs[b]) and rs[b:b + 1].view(np.uint64)[0] != MARKER_BITS:
                    assert np.isnan(g[b][m[b]]).all(), (what, k, b)
                elif np.isnan(rs[b]):
                    assert not g[b].any(), (what, k, b)
                continue
            if np.isneginf(rs[b]):
                assert not g[b].any(), (what, k, b, "no path: exact zeros")
                continue
            if k in ("hx", "hy"):
                mag = np.abs(r[b])
            else:
                mag = abs(ge[b]) * ref["mag" + k[1]][b] + abs(gs[b]) * ref["occ" + k[1]][b]
            res = O.grad_check(g[b], r[b], mag, name)
            assert res["passed"], (what, k, b, res)
            worst = max(worst, res["max_err_over_quantum"])
    print(what, "worst error / bound = %.3e" % worst)
    return worst


def _same(a, b, keys):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


ALL = ("scores", "expect", "nodes") + GRADS


# ----------------------------------------------------------------------------- every form of tests/expect_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_expect_form(name):
    case = F.CASES[name]
    px, py, cx, cy, bd, mx, my = _table_problem(case)
    dv = _dev(px, py, cx, cy)
    run = lambda: call(*dv, bd, "all")                                                       # noqa: E731
    got, names = profiled(run)
    if got["st"] == 0 and not names:                 # (a profiler session now and then records no device event at all:
        got, names = profiled(run)                   #  one more session, judged as the first would have been)
    assert got["st"] == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, G.cus()))
    ref = _reference(px, py, cx, cy, bd, case["mod"])
    _check(got, ref, case["dtype"], mx, my, what=name)
    if case["N"] >= F.PATTERNS:
        rsc = ref["scores"]
        assert np.isfinite(rsc[3]) and (case["mod"] or np.isfinite(rsc).all()), rsc
        if case["mod"] and case["S"] > 0:
            assert np.isneginf(rsc[6]) and np.isfinite(rsc[5]), rsc


def test_every_expect_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- negative control
@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", False), ("f16", True)])
def test_negative_control_another_boundary_is_refused(dtype, mod):
    """The result with one boundary against the reference with another must fail the identical _check: the checks cannot pass
    on a library that ignores the boundary."""
    N, S, T = 4, 5, 9
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 8], [0, 1, 3, 9], [2, 0, 5, 7]], np.int64)
    other = np.array([[0, 1, 5, 9], [1, 2, 4, 7], [0, 1, 4, 9], [1, 0, 5, 7]], np.int64)
    px, py, cx, cy, bd, mx, my = _problem("neg", dtype, N, S, T, mod, bd, poison_outside=False)
    got = call(*_dev(px, py, cx, cy), bd)
    assert got["st"] == 0
    _check(got, _reference(px, py, cx, cy, bd, mod), dtype, mx, my, what="own boundary")
    omx, omy = R.edge_masks(N, S, T, mod, other)
    with pytest.raises(AssertionError):
        _check(got, _reference(px, py, cx, cy, other, mod), dtype, omx, omy, what="another boundary")
    oth = _reference(px, py, cx, cy, other, mod)
    own = _reference(px, py, cx, cy, bd, mod)
    for k in ("scores", "expect"):                       # each scalar on its own, too
        with pytest.raises(AssertionError):
            _check(dict(got, gx=None), dict(own, **{k: oth[k]}), dtype, mx, my, what="another " + k)


# ----------------------------------------------------------------------------- call forms and reruns
@pytest.mark.parametrize("dtype,S,mod", [("f32", 8, False), ("bf16", 8, True), ("f32", 65, True), ("f64", 69, False),
                                         ("f16", 130, False)])
def test_call_forms_agree(dtype, S, mod):
    """one / two-phase / host scalars / forward-only / without cost gradients: bit for bit where they compute the same thing;
    per-sample scales; costs aliasing weights; a second run gives the same bits."""
    N, T = 7, 75 if mod else 11
    case = dict(name="forms_%s_%d" % (dtype, S), dtype=dtype, N=N, S=S, T=T, mod=mod)
    px, py, cx, cy, bd, mx, my = _table_problem(case, seed=S)
    dv = _dev(px, py, cx, cy)
    one = call(*dv, bd)
    assert one["st"] == 0
    _check(one, _reference(px, py, cx, cy, bd, mod), dtype, mx, my, what="one call")
    again = call(*dv, bd)
    assert again["st"] == 0 and _same(one, again, ALL)
    two, names = profiled(lambda: call(*dv, bd, "two"))                                      # NULL scales: 1 and 0
    assert two["st"] == 0 and _same(one, two, ALL)
    assert not names or stages_seen(names, F.stage_of, F.STAGES) == F.predict(case)
    fwd, names = profiled(lambda: call(*dv, bd, "fwdonly"))
    assert fwd["st"] == 0 and _same(one, fwd, ALL[:3])
    seen = stages_seen(names, F.stage_of, F.STAGES)
    assert not names or (seen["fwd"] == F.predict(case)["fwd"] and not seen["bwd"] and not seen["restore"]), seen
    host, names = profiled(lambda: call(*dv, bd, "host"))
    assert host["st"] == 0 and _same(one, host, ALL)
    assert not names or stages_seen(names, F.stage_of, F.STAGES) == F.predict(case, host=True)
    noc, names = profiled(lambda: call(*dv, bd, "nocost"))
    assert noc["st"] == 0 and _same(one, noc, ALL[:5])
    assert not names or stages_seen(names, F.stage_of, F.STAGES) == F.predict(case, cost_grads=False)
    # per-sample scales, both non-trivial
    ge, gs = 0.5 + 0.25 * np.arange(N), 0.75 - 0.5 * np.arange(N)
    ge[1] = -1.5
    sc = call(*dv, bd, "two", ge=ge, gs=gs)
    assert sc["st"] == 0 and _same(one, sc, ALL[:3])
    _check(sc, _reference(px, py, cx, cy, bd, mod, ge, gs), dtype, mx, my, ge, gs, what="scaled")
    snc = call(*dv, bd, "two_nocost", ge=ge, gs=gs)
    assert snc["st"] == 0 and _same(sc, snc, ALL[:5])
    # g_expect = 0, g_score = 1: the occupations, cx_grad = 0
    occ = call(*dv, bd, "two", ge=np.zeros(N), gs=np.ones(N))
    ref = _reference(px, py, cx, cy, bd, mod, np.zeros(N), np.ones(N))
    _check(occ, ref, dtype, mx, my, np.zeros(N), np.ones(N), what="occupations")
    assert not occ["hx"].any() and not occ["hy"].any()
    # costs aliasing weights: the entropy's call
    al = call(dv[0], dv[1], dv[0], dv[1], bd)
    assert al["st"] == 0
    _check(al, _reference(px, py, px, py, bd, mod), dtype, mx, my, what="c = w")


# ----------------------------------------------------------------------------- the header's edge cases
def _edge_problem(dtype, mod):
    N, S, T = 8, 4, 7
    bd = R.full_boundary(N, S, T)
    bd[3] = (1, 1, 3, 6)
    bd[6] = (0, 2, 4, 7)
    return _problem("nf", dtype, N, S, T, mod, bd, poison_outside=False)


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("mod", [False, True])
def test_no_path_and_infinite_edges(dtype, mod):
    """-inf holes with a path around them, with NaN and -inf costs on them (never looked at); no path: score -inf, expect 0,
    exact zeros."""
    px, py, cx, cy, bd, mx, my = _edge_problem(dtype, mod)
    T = py.shape[2]
    px[0, 1, 2] = NEG
    cx[0, 1, 2] = float("nan")
    py[0, 2, 3] = NEG
    cy[0, 2, 3] = NEG
    py[0, 0, 0] = NEG
    cy[0, 0, 0] = float("inf")
    if not mod:
        px[0, :, T] = NEG                               # k2's own -inf column
        cx[0, :, T] = float("nan")
    px[1, 2, :] = NEG                                   # symbol 2 can never be emitted: no path
    got = call(*_dev(px, py, cx, cy), bd)
    assert got["st"] == 0
    ref = _reference(px, py, cx, cy, bd, mod)
    assert np.isfinite(ref["scores"][0]) and np.isfinite(ref["expect"][0]) and np.isneginf(ref["scores"][1])
    _check(got, ref, dtype, mx, my, what="holes")
    assert np.isneginf(got["scores"][1]) and got["expect"][1] == 0
    for k in GRADS:
        assert not got[k][1].any(), k


@pytest.mark.parametrize("mod", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_weight_poisons_its_sample_alone(mod, bad):
    px, py, cx, cy, bd, mx, my = _edge_problem("f32", mod)
    px[3, 1, 3] = bad                                   # inside sample 3's rectangle
    py[4, 4, 6] = bad
    px[5, 0, 0] = bad
    py[6, 0, 0] = bad                                   # outside sample 6's rectangle (t0 = 2): nothing changes
    got = call(*_dev(px, py, cx, cy), bd)
    assert got["st"] == 0
    ref = _reference(px, py, cx, cy, bd, mod)
    assert np.isnan(ref["scores"][3:6]).all() and np.isfinite(ref["scores"][[0, 1, 2, 6, 7]]).all()
    _check(got, ref, "f32", mx, my, what="poisoned")
    for b in (3, 4, 5):
        assert np.isnan(got["scores"][b]) and np.isnan(got["expect"][b])
        for k, m in zip(GRADS, (mx, my, mx, my)):
            assert np.isnan(got[k][b][m[b]]).all() and not got[k][b][~m[b]].any(), (k, b)


@pytest.mark.parametrize("mod", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_cost_on_a_finite_edge(mod, bad):
    """expect NaN for that sample alone; its score, and its gradients bit for bit on a rerun."""
    px, py, cx, cy, bd, mx, my = _edge_problem("f64", mod)
    cx[2, 1, 3] = bad
    cy[4, 2, 2] = bad
    dv = _dev(px, py, cx, cy)
    got, again = call(*dv, bd), call(*dv, bd)
    assert got["st"] == 0 and _same(got, again, ALL)
    ref = _reference(px, py, cx, cy, bd, mod)
    assert np.isnan(ref["expect"][[2, 4]]).all() and np.isfinite(ref["scores"]).all()
    _check(got, ref, "f64", mx, my, what="bad costs")
    assert np.isnan(got["expect"][[2, 4]]).all() and np.isfinite(got["expect"][[0, 1, 3, 5, 6, 7]]).all()


@pytest.mark.parametrize("mod", [False, True])
def test_degenerate_rectangles(mod):
    """fp64.  s1 == s0: the frames alone, expect the sum of cy; t1 == t0: regular the symbols at t0, modified 0 paths unless
    s1 == s0; modified with s1 - s0 == t1 - t0: the diagonal of px; S = 0: px, cx and their gradients have no element."""
    N, S, T = 5, 3, 6
    bd = np.array([[2, 1, 2, 5], [0, 4, 3, 4], [1, 3, 1, 3], [0, 2, 3, 5], [0, 0, 3, 6]], np.int64)
    px, py, cx, cy, bd, mx, my = _problem("deg", "f64", N, S, T, mod, bd)
    got = call(*_dev(px, py, cx, cy), bd)
    assert got["st"] == 0
    _check(got, _reference(px, py, cx, cy, bd, mod), "f64", mx, my, what="degenerate")
    X, Y, CX, CY = (_stored(t) for t in (px, py, cx, cy))
    assert got["scores"][0] == pytest.approx(Y[0, 2, 1:5].sum(), rel=1e-12)
    assert got["expect"][0] == pytest.approx(CY[0, 2, 1:5].sum(), rel=1e-12, abs=1e-12)
    assert got["scores"][2] == 0 and got["expect"][2] == 0
    if mod:
        assert np.isneginf(got["scores"][1]) and got["expect"][1] == 0
        assert got["expect"][3] == pytest.approx(sum(CX[3, i, 2 + i] for i in range(3)), rel=1e-12, abs=1e-12)
    else:
        assert got["expect"][1] == pytest.approx(CX[1, :, 4].sum(), rel=1e-12, abs=1e-12)
    p0 = _problem("s0", "f64", 3, 0, 9, mod, np.array([[0, 0, 0, 9], [0, 3, 0, 4], [0, 5, 0, 5]]))
    for form in ("all", "host", "fwdonly", "two"):
        got = call(*_dev(*p0[:4]), p0[4], form)
        assert got["st"] == 0
        _check(got, _reference(*p0[:5], mod), "f64", p0[5], p0[6], what="S = 0 " + form)
        if form != "fwdonly":
            assert got["gx"].size == 0 and got["hx"].size == 0 and np.array_equal(got["hy"], p0[6].astype(np.float64))


def test_invalid_arguments_and_limits():
    """A boundary outside the tensor: the marker (INVALID_VALUE with host scalars), expect 0, gradients 0, the other samples
    untouched; every refusal of the header returns INVALID_VALUE with the outputs untouched."""
    lib = _ex().lib()
    N, S, T = 3, 4, 6
    px, py, cx, cy, bd, mx, my = _problem("inv", "f32", N, S, T, False, poison_outside=False)
    dv = _dev(px, py, cx, cy)
    good = call(*dv, None)
    assert good["st"] == 0 and np.isfinite(good["scores"]).all()
    for row in ((0, 0, S + 1, T), (0, 0, S, T + 1), (-1, 0, S, T), (0, -1, S, T), (3, 0, 2, T), (0, 5, S, 4),
                (0, 0, 2 ** 40, T), (-2 ** 62, 0, S, T)):
        bad = R.full_boundary(N, S, T)
        bad[1] = row
        for mod in (False, True):
            d2 = [dv[0][:, :, :T].contiguous(), dv[1], dv[2][:, :, :T].contiguous(), dv[3]] if mod else dv
            assert call(*d2, bad, "host")["st"] == 2, row
            got = call(*d2, bad)
            assert got["st"] == 0 and got["scores"][1:2].view(np.uint64)[0] == MARKER_BITS and got["expect"][1] == 0, row
            assert all(not got[k][1].any() for k in GRADS)
            assert np.isneginf(got["nodes"][1, ..., 0]).all() and not got["nodes"][1, ..., 1].any()
            if not mod:
                assert _same({k: good[k][[0, 2]] for k in ALL}, {k: got[k][[0, 2]] for k in ALL}, ALL)
    nan = float("nan")
    scores = torch.full((N,), nan, dtype=torch.float64, device=DEV)
    expect = torch.full((N,), nan, dtype=torch.float64, device=DEV)
    nodes = torch.full((N, S + 1, T + 1, 2), nan, dtype=torch.float64, device=DEV)
    g = {k: torch.full_like(dv[i % 2], nan) for i, k in enumerate(GRADS)}
    outs = [scores, expect, nodes] + list(g.values())
    xd, yd, cxd, cyd = dv
    one = lambda **kw: lib.compute_rnnt_expect(                                                          # noqa: E731
        kw.get("px", xd.data_ptr()), kw.get("py", yd.data_ptr()), kw.get("cx", cxd.data_ptr()), kw.get("cy", cyd.data_ptr()),
        None, kw.get("S", S), kw.get("T", T), kw.get("N", N), 0, kw.get("scores", scores.data_ptr()),
        kw.get("expect", expect.data_ptr()), kw.get("nodes", nodes.data_ptr()), kw.get("gx", g["gx"].data_ptr()),
        kw.get("gy", g["gy"].data_ptr()), kw.get("hx", g["hx"].data_ptr()), kw.get("hy", g["hy"].data_ptr()),
        kw.get("opt", _opt()), kw.get("code", 0))
    cpu = _opt()
    cpu.loc = 0
    refused = [dict(px=None), dict(py=None), dict(cx=None), dict(cy=None), dict(scores=None), dict(expect=None), dict(nodes=None),
               dict(gx=None), dict(gy=None), dict(hx=None), dict(hy=None), dict(gx=None, gy=None), dict(code=4), dict(code=-1),
               dict(opt=cpu), dict(S=-1), dict(T=0), dict(N=0), dict(S=1024), dict(S=1023, T=(1 << 15) - 1),
               dict(S=15, T=(1 << 12) - 1, N=1 << 16), dict(gx=xd.data_ptr()), dict(gy=cyd.data_ptr()), dict(hx=cxd.data_ptr()),
               dict(hy=yd.data_ptr() + 16), dict(hx=g["gx"].data_ptr()), dict(gx=g["gx"].data_ptr() + 2),
               dict(nodes=nodes.data_ptr() + 8), dict(nodes=scores.data_ptr()), dict(scores=expect.data_ptr()),
               dict(expect=g["gy"].data_ptr()), dict(scores=scores.data_ptr() + 4)]
    for kw in refused:
        assert one(**kw) == 2, kw
    bwd = lambda **kw: lib.compute_rnnt_expect_bwd(                                                      # noqa: E731
        kw.get("px", xd.data_ptr()), yd.data_ptr(), cxd.data_ptr(), kw.get("cy", cyd.data_ptr()), None,
        kw.get("nodes", good_nodes.data_ptr()), kw.get("scores", good_scores.data_ptr()), good_expect.data_ptr(), None, None,
        kw.get("S", S), T, N, 0, kw.get("gx", g["gx"].data_ptr()), kw.get("gy", g["gy"].data_ptr()),
        kw.get("hx", g["hx"].data_ptr()), kw.get("hy", g["hy"].data_ptr()), kw.get("opt", _opt()), kw.get("code", 0))
    good_nodes, good_scores, good_expect = (torch.tensor(good[k], device=DEV) for k in ("nodes", "scores", "expect"))
    for kw in (dict(px=None), dict(cy=None), dict(nodes=None), dict(scores=None), dict(gx=None), dict(gy=None), dict(hx=None),
               dict(hy=None), dict(code=7), dict(opt=cpu), dict(S=1024), dict(gx=good_nodes.data_ptr()),
               dict(gy=good_scores.data_ptr()), dict(hx=g["gx"].data_ptr())):
        assert bwd(**kw) == 2, kw
    fwd = lambda **kw: lib.compute_rnnt_expect_fwd(                                                      # noqa: E731
        xd.data_ptr(), kw.get("py", yd.data_ptr()), cxd.data_ptr(), cyd.data_ptr(), None, kw.get("S", S), T, N, 0,
        kw.get("scores", scores.data_ptr()), kw.get("expect", expect.data_ptr()), kw.get("nodes", nodes.data_ptr()), _opt(),
        kw.get("code", 0))
    for kw in (dict(py=None), dict(scores=None), dict(expect=None), dict(nodes=None), dict(S=1024), dict(code=4),
               dict(nodes=yd.data_ptr()), dict(expect=scores.data_ptr())):
        assert fwd(**kw) == 2, kw
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in outs)                                           # untouched
    assert one() == 0 and one(hx=None, hy=None) == 0 and one(gx=None, gy=None, hx=None, hy=None) == 0
    assert bwd() == 0 and bwd(hx=None, hy=None) == 0 and fwd() == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- against this tree
@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", True), ("f16", False)])
def test_scores_and_occupations_are_mi(dtype, mod):
    """scores against mutual_information_recursion's at COST_TOL[dtype]; cx_grad against its px_grad at oracle.grad_bound of
    the dtype (the project's tolerances for `mi`)."""
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    case = dict(name="mi_%s" % dtype, dtype=dtype, N=7, S=20, T=33, mod=mod)
    px, py, cx, cy, bd, mx, my = _table_problem(case, seed=11)
    dv = _dev(px, py, cx, cy)
    got = call(*dv, bd)
    sc, (ox, oy) = mir(dv[0], dv[1], torch.tensor(bd, device=DEV), return_grad=True)
    sc, ox, oy = sc.double().cpu().numpy(), ox.double().cpu().numpy(), oy.double().cpu().numpy()
    fin = np.isfinite(got["scores"])
    assert np.array_equal(np.isneginf(sc), np.isneginf(got["scores"]))
    tol = COST_TOL[dtype]
    print("max |dscore| =", np.abs(sc[fin] - got["scores"][fin]).max())
    assert np.allclose(sc[fin], got["scores"][fin], rtol=tol, atol=tol)
    for mine, theirs in ((got["hx"], ox), (got["hy"], oy)):
        err, bound = np.abs(mine - theirs), O.grad_bound(mine, np.abs(mine), _BOUND_DTYPE[dtype])
        print("max occupation error / bound =", (err / bound).max(initial=0))
        assert (err <= bound).all()


# ----------------------------------------------------------------------------- the Python module
def test_python_validation_on_the_device():
    from warprnnt_pytorch.expect import alignment_entropy, expected_cost
    px, py = torch.zeros(2, 3, 6, device=DEV), torch.zeros(2, 4, 5, device=DEV)
    cx, cy = torch.ones_like(px), torch.ones_like(py)
    for row in ((0, 0, 4, 5), (0, 0, 3, 6), (2, 0, 1, 5), (0, -1, 3, 5)):
        bd = torch.tensor([[0, 0, 3, 5], row], device=DEV)
        with pytest.raises(ValueError, match="boundary\\[1\\]"):
            expected_cost(px, py, cx, cy, bd)
        ec, sc = expected_cost(px, py, cx, cy, bd, return_scores=True, validate=False)       # enqueue only: the sample is marked
        assert torch.isnan(sc[1]) and torch.isfinite(sc[0]) and ec[1] == 0 and ec[0] == 8
    with pytest.raises(ValueError, match="one device"):
        expected_cost(px, py, cx, cy, torch.tensor([[0, 0, 3, 5]] * 2))
    with pytest.raises(ValueError, match="device of px"):
        expected_cost(px, py, cx.cpu(), cy)
    with pytest.raises(ValueError, match="shape and dtype of py"):
        expected_cost(px, py, cx, cy.double())
    with pytest.raises(ValueError, match="shape and dtype of px"):
        expected_cost(px, py, cx[:, :, :5].contiguous(), cy)
    for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        ec, sc = expected_cost(px.to(dt), py.to(dt), cx.to(dt), cy.to(dt), return_scores=True)
        assert ec.dtype == sc.dtype == torch.float64 and ec.shape == sc.shape == (2,)
        assert torch.allclose(ec, torch.full_like(ec, 8.0), rtol=1e-12)                      # every path has 3 + 5 edges
        h = alignment_entropy(px.to(dt), py.to(dt))
        assert torch.allclose(h, sc, rtol=1e-12)                                             # uniform: log(number of paths)
    assert expected_cost(px[:, :, :5].contiguous(), py, cx[:, :, :5].contiguous(), cy).tolist() == [5.0, 5.0]


@pytest.mark.parametrize("mod", [False, True])
def test_gradcheck_fp64(mod):
    from warprnnt_pytorch.expect import alignment_entropy, expected_cost
    rng = np.random.default_rng(2)
    B, S, T = 3, 2, 4
    mk = lambda shape, off: torch.tensor(rng.standard_normal(shape) + off, dtype=torch.float64, device=DEV,    # noqa: E731
                                         requires_grad=True)
    px, py = mk((B, S, T if mod else T + 1), -1), mk((B, S + 1, T), -1)
    cx, cy = mk(px.shape, 0), mk(py.shape, 0)
    bd = torch.tensor([[0, 0, 2, 4], [1, 1, 2, 4], [0, 0, 2, 3]], device=DEV)
    kw = dict(eps=1e-6, atol=1e-6, nondet_tol=1e-12)
    assert torch.autograd.gradcheck(lambda a, b, c, d: expected_cost(a, b, c, d, bd), (px, py, cx, cy), **kw)
    assert torch.autograd.gradcheck(lambda a, b, c, d: expected_cost(a, b, c, d, bd, return_scores=True), (px, py, cx, cy), **kw)
    assert torch.autograd.gradcheck(lambda a, b: expected_cost(a, b, cx.detach(), cy.detach(), bd), (px, py), **kw)
    assert torch.autograd.gradcheck(lambda a, b: alignment_entropy(a, b, bd), (px, py), **kw)


@pytest.mark.parametrize("mod", [False, True])
def test_autograd_launches_and_skips_cost_gradients(mod):
    """One forward and one backward launch per call; the backward without cost gradients when neither cost needs one; the
    entropy's gradient is the sum of the two gradients of the c = w call."""
    from warprnnt_pytorch.expect import alignment_entropy, expected_cost
    case = dict(name="ag", dtype="f32", N=7, S=9, T=14, mod=mod)
    px, py, cx, cy, bd, mx, my = _table_problem(case, seed=3)
    clean = lambda t: torch.nan_to_num(t, nan=-1.0).to(DEV)                                  # noqa: E731  (autograd adds the tensors)
    xd, yd, cxd, cyd = (clean(t) for t in (px, py, cx, cy))
    bt = torch.tensor(bd, device=DEV)
    go = torch.tensor([0.7, -1.3, 2.0, 1.0, 0.25, 3.0, -0.5], dtype=torch.float64, device=DEV)
    xa, ya = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    ec = expected_cost(xa, ya, cxd, cyd, bt)
    _, names = profiled(lambda: (ec * go).sum().backward())
    seen = stages_seen(names, F.stage_of, F.STAGES)
    assert not names or seen == dict(F.predict(case, cost_grads=False), fwd=set()), seen
    ref = R.expected_cost(_stored(xd), _stored(yd), _stored(cxd), _stored(cyd), bd, mod, go.cpu().numpy())
    got = dict(gx=xa.grad.double().cpu().numpy(), gy=ya.grad.double().cpu().numpy())
    for k, m in (("gx", mx), ("gy", my)):
        for b in range(7):
            mag = abs(go[b].item()) * ref["mag" + k[1]][b]
            assert O.grad_check(got[k][b], ref[k][b], mag, "float32")["passed"], (k, b)
        assert not got[k][~m].any()
    xb, yb = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    (h, names) = profiled(lambda: alignment_entropy(xb, yb, bt))
    seen = stages_seen(names, F.stage_of, F.STAGES)
    assert not names or seen == dict(F.predict(case), bwd=set()), seen
    _, names = profiled(lambda: (h * go).sum().backward())
    seen = stages_seen(names, F.stage_of, F.STAGES)
    assert not names or seen == dict(F.predict(case), fwd=set()), seen
    X, Y = _stored(xd), _stored(yd)
    ref = R.expected_cost(X, Y, X, Y, bd, mod, -go.cpu().numpy(), go.cpu().numpy())
    fin = np.isfinite(ref["scores"])
    assert np.allclose(h.detach().cpu().numpy()[fin], (ref["scores"] - ref["expect"])[fin], rtol=1e-9, atol=1e-9)
    for k, hk, grad in (("gx", "hx", xb.grad), ("gy", "hy", yb.grad)):
        want = ref[k] + ref[hk]                          # d H / d w = g_score occ - (occ dev + occ) at g_expect = -go
        mag = np.abs(go.cpu().numpy()).reshape(-1, 1, 1) * (ref["mag" + k[1]] + 2 * ref["occ" + k[1]])
        res = O.grad_check(grad.double().cpu().numpy()[fin], want[fin], mag[fin], "float32")
        assert res["passed"], (k, res)


def test_hip_graph_capture_and_replay():
    """validate=False forward + backward captured once on one stream (one branch), replayed twice on new inputs."""
    from warprnnt_pytorch.expect import expected_cost
    B, S, T = 3, 5, 9
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 9], [0, 0, 3, 6]], np.int64)
    bt = torch.tensor(bd, device=DEV)
    mk = lambda *shape: torch.zeros(shape, device=DEV, requires_grad=True)                   # noqa: E731
    sx, sy, scx, scy = mk(B, S, T + 1), mk(B, S + 1, T), mk(B, S, T + 1), mk(B, S + 1, T)
    leaves = (sx, sy, scx, scy)
    _ex().lib()

    def step():
        for t in leaves:
            t.grad = None
        ec, sc = expected_cost(sx, sy, scx, scy, bt, return_scores=True, validate=False)
        (ec + 0.5 * sc).sum().backward()
        return ec, sc

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for t in leaves:
        t.grad = None
    with torch.cuda.graph(graph):
        ec, sc = step()
    grads = [t.grad for t in leaves]
    mx, my = R.edge_masks(B, S, T, False, bd)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        vals = [(rng.standard_normal(t.shape) - (1 if i < 2 else 0)).astype(np.float32) for i, t in enumerate(leaves)]
        with torch.no_grad():
            for t, v in zip(leaves, vals):
                t.copy_(torch.tensor(v))
        graph.replay()
        torch.cuda.synchronize()
        ref = R.expected_cost(*vals, bd, False, np.ones(B), np.full(B, 0.5))
        got = dict(st=0, scores=sc.detach().cpu().numpy(), expect=ec.detach().cpu().numpy(), nodes=ref["nodes"],
                   **{k: g.double().cpu().numpy() for k, g in zip(GRADS, grads)})
        _check(got, ref, "f32", mx, my, np.ones(B), np.full(B, 0.5), what="replay %d" % seed)


# ----------------------------------------------------------------------------- a large batch, long lattices
def test_large_batch():
    """B = 65537 > 65535, S = 1, T = 2, regular, fp32: the sample rides on grid.x.  The last two samples against the
    reference, every sample finite, and the first 1000 samples equal the same call on them alone."""
    B, S, T = 65537, 1, 2
    rng = np.random.default_rng(65537)
    px = torch.tensor(rng.standard_normal((B, S, T + 1)) - 1.5, dtype=torch.float32)
    py = torch.tensor(rng.standard_normal((B, S + 1, T)) - 1.5, dtype=torch.float32)
    cx = torch.tensor(rng.standard_normal((B, S, T + 1)), dtype=torch.float32)
    cy = torch.tensor(rng.standard_normal((B, S + 1, T)), dtype=torch.float32)
    dv = _dev(px, py, cx, cy)
    got = call(*dv, None)
    assert got["st"] == 0 and np.isfinite(got["scores"]).all() and np.isfinite(got["expect"]).all()
    tail = slice(B - 2, B)
    ref = _reference(px[tail], py[tail], cx[tail], cy[tail], None, False)
    mx, my = R.edge_masks(2, S, T, False)
    _check({k: (got[k] if k == "st" else got[k][tail]) for k in got}, ref, "f32", mx, my, what="the last two of 65537")
    head = call(*[t[:1000].contiguous() for t in dv], None)
    assert _same({k: got[k][:1000] for k in ALL}, head, ALL)


@pytest.mark.parametrize("S,mod", [(1023, False), (32, False), (1023, True), (32, True)])
def test_long_lattice(S, mod):
    """One long lattice per form at N = 2, T = 128 (modified at S = 1023: T = 1100, room for the symbols), fp32: drift over
    ~1150 steps stays inside the same bounds.  The second sample is a short rectangle inside."""
    N, T = 2, (1100 if S > 128 else 128) if mod else 128
    bd = np.array([[0, 0, S, T], [3, 40, min(S, 33), 120]], np.int64)
    px, py, cx, cy, bd, mx, my = _problem("long", "f32", N, S, T, mod, bd)
    got = call(*_dev(px, py, cx, cy), bd)
    assert got["st"] == 0
    ref = _reference(px, py, cx, cy, bd, mod)
    assert np.isfinite(ref["scores"]).all()
    _check(got, ref, "f32", mx, my, what="long S = %d" % S)
