"""-m gpu: the best path over px / py edge log-probabilities (include/rnnt_bestpath.h, libwarprnnt_bestpath.so).

Every case of tests/bestpath_forms.py runs through compute_rnnt_bestpath under torch.profiler with all outputs taken: exactly
the kernels its release rule predicts run, stage by stage.  scores, frames and back EQUAL those of the numpy fp64 reference
of tests/bestpath_ref.py (np.array_equal: the header fixes every addition, so there is no tolerance); px_path / py_path equal
the reference's indicators exactly, and their dot product with the inputs is the path's weight within the bound of a
sequential fp64 sum.  Inputs are NaN outside the rectangles' edge sets (never read); outputs are prefilled with NaN, -7 and
0xFF (every element is written) and sit between 4096 guard bytes that stay as they were.  The reference is given the stored
values.

Then: exact ties on the device, two negative controls (another boundary; the symbol edge on ties), rnnt_align and
mutual_information_recursion of this tree as yardsticks, the call forms, the header's edge cases, the invalid arguments and
limits, the Python module with autograd and a HIP-graph capture, and two long lattices."""
import math
import zlib

import numpy as np
import pytest
import torch

from tests import bestpath_forms as F
from tests import bestpath_ref as R
from tests import gpu_support as G
from tests.gpu_support import CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, profiled, stages_seen
from tests.test_bestpath_cpu import tie_case

pytestmark = pytest.mark.gpu
NEG = float("-inf")
GUARD = 4096


def _bp():
    from warprnnt_pytorch import bestpath
    return bestpath


def _opt(stream=None):
    return G.options(1, 1, 0, stream)                   # (only loc and stream are read)


def _problem(name, dtype, N, S, T, mod, bd=None, rng=None, poison_outside=True):
    """px, py of the storage type on the CPU: weights around -1.5, NaN outside every rectangle's edge sets; the boundary rows
    and the two edge masks."""
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


class Guarded:
    """A device buffer of `shape` between two runs of GUARD bytes of 0xA5, its elements prefilled with `fill`."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.n = n
        self.raw = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(shape)
        self.t.fill_(fill)
        self.ptr = self.t.data_ptr() if n else None

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all() and (self.raw[GUARD + self.n:] == 0xA5).all())


def call(px, py, bd=None, form="all", scale=None, prev=None, stream=None):
    """One C-ABI call on device tensors -> dict(st, scores, frames, back, ex, ey) as numpy (ex, ey float64; None where the
    form has none).  form: all (device scores, indicators) | noedges | host (host scores, indicators) | edges (the second
    entry on the frames and scores of `prev`, with `scale`).  Every output starts as NaN / -7 / 0xFF between guards."""
    m = _bp()
    lib = m.lib()
    N, S1, T = py.shape
    S, mod = S1 - 1, int(px.shape[2] == T)
    code = CODE[NAME[py.dtype]]
    bt = None if bd is None else torch.tensor(np.asarray(bd, np.int64), device=DEV)
    bp = None if bt is None else bt.data_ptr()
    xp = px.data_ptr() if px.numel() else None
    opt = _opt(stream)
    gs = Guarded((N,), torch.float64, float("nan"))
    gf = Guarded((N, S), torch.int32, -7)
    gb = Guarded((N, S + 1, R.back_words(T)), torch.int64, -1)
    gx = Guarded(tuple(px.shape), px.dtype, float("nan"))
    gy = Guarded(tuple(py.shape), py.dtype, float("nan"))
    used = [gx, gy]
    if form == "edges":
        fr = torch.tensor(prev["frames"], device=DEV)
        sc = torch.tensor(prev["scores"], device=DEV)
        st_scale = None if scale is None else torch.tensor(np.asarray(scale, np.float64), device=DEV)
        st = lib.compute_rnnt_bestpath_edges(fr.data_ptr() if fr.numel() else None, sc.data_ptr(), bp,
                                             None if st_scale is None else st_scale.data_ptr(), S, T, N, mod, gx.ptr, gy.ptr,
                                             opt, code)
        torch.cuda.synchronize()
        out = dict(st=st, scores=prev["scores"], frames=prev["frames"], back=prev["back"])
    else:
        used += [gf, gb]
        edges = form != "noedges"
        if form == "host":
            hs = np.full(N, np.nan)
            sptr = hs.ctypes.data
        else:
            used.append(gs)
            sptr = gs.ptr
        st = lib.compute_rnnt_bestpath(xp, py.data_ptr(), bp, S, T, N, mod, sptr, gf.ptr, gb.ptr, gx.ptr if edges else None,
                                       gy.ptr if edges else None, opt, code)
        torch.cuda.synchronize()
        out = dict(st=st, scores=hs if form == "host" else gs.t.cpu().numpy(), frames=gf.t.cpu().numpy(),
                   back=gb.t.cpu().numpy().view(np.uint64))
        if not edges:
            assert torch.isnan(gx.t).all() and torch.isnan(gy.t).all()                       # not taken: not touched
    for g in used:
        assert g.guards_intact()
    has = form != "noedges"
    out["ex"] = gx.t.double().cpu().numpy() if has else None
    out["ey"] = gy.t.double().cpu().numpy() if has else None
    return out


def _stored(t):
    return t.double().cpu().numpy()


def _reference(px, py, bd, mod, strict=True):
    return R.best_path(_stored(px), _stored(py), bd, mod, strict)


def _same(got, ref, what=""):
    """scores, frames and back against the reference's: equal, -inf position for position (NaN where it has NaN)."""
    rsc, rfr, rbk = ref
    assert np.array_equal(got["scores"], rsc, equal_nan=True), (what, got["scores"], rsc)
    assert np.array_equal(got["frames"], rfr), (what, "frames")
    assert np.array_equal(got["back"], rbk), (what, "back")


def _check_edges(got, px, py, bd, mod, scale=None, what=""):
    """px_path / py_path equal the reference's indicators exactly; at scale 1 their dot product with the inputs is the path's
    weight within n 2^-53 sum |w| (n edges on the path): the bound of a sequential fp64 sum against the exact one."""
    N, S1, T = py.shape
    ex, ey = R.edges(got["frames"], got["scores"], bd, S1 - 1, T, mod, scale)
    assert np.array_equal(got["ex"], ex, equal_nan=True), (what, "px_path")
    assert np.array_equal(got["ey"], ey, equal_nan=True), (what, "py_path")
    if scale is not None:
        return
    X, Y = _stored(px), _stored(py)
    rs = R.rescore(X, Y, bd, mod, got["frames"])
    worst = 0.0
    for b in range(N):
        if not np.isfinite(got["scores"][b]):
            continue
        on_x, on_y = got["ex"][b] != 0, got["ey"][b] != 0
        dot = math.fsum(list(X[b][on_x] * got["ex"][b][on_x]) + list(Y[b][on_y] * got["ey"][b][on_y]))
        acc, n, mag = rs[b]
        assert int(on_x.sum() + on_y.sum()) == int(n), (what, b)
        bound = n * 2.0 ** -53 * mag
        print(what, "sample %d: |dot - rescore| = %.3e, bound %.3e" % (b, abs(dot - acc), bound))
        assert abs(dot - acc) <= bound, (what, b, dot, acc, bound)
        assert got["scores"][b] == acc, (what, b)                                             # the sweep adds in path order too
        worst = max(worst, abs(dot - acc) / bound if bound else 0.0)
    return worst


def _mir_bound(px, py, bd, mod, dtype, scores, what=""):
    """mir - log(n_paths) - tol <= score <= mir + tol for every sample with a path, tol = COST_TOL (1 + |mir|)."""
    from warprnnt_pytorch.mi import mutual_information_recursion
    mir = mutual_information_recursion(px.to(DEV), py.to(DEV), torch.tensor(bd, device=DEV)).double().cpu().numpy()
    for b, (s0, t0, s1, t1) in enumerate(np.asarray(bd)):
        Sr, Tr = int(s1 - s0), int(t1 - t0)
        n_paths = math.comb(Tr, Sr) if mod else math.comb(Sr + Tr, Sr)
        if not np.isfinite(scores[b]):
            assert n_paths == 0 and np.isneginf(mir[b]), (what, b)
            continue
        tol = COST_TOL[dtype] * (1 + abs(mir[b]))
        print(what, "sample %d: mir %.6f score %.6f paths %d" % (b, mir[b], scores[b], n_paths))
        assert mir[b] - math.log(n_paths) - tol <= scores[b] <= mir[b] + tol, (what, b, mir[b], scores[b], n_paths)


# ----------------------------------------------------------------------------- every form of tests/bestpath_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_bestpath_form(name):
    case = F.CASES[name]
    px, py, bd, mx, my = _table_problem(case)
    xd, yd = px.to(DEV), py.to(DEV)
    run = lambda: call(xd, yd, bd, "all")                                                    # noqa: E731
    got, names = profiled(run)
    if got["st"] == 0 and not names:                 # (a profiler session now and then records no device event at all:
        got, names = profiled(run)                   #  one more session, judged as the first would have been)
    assert got["st"] == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, G.cus()))
    ref = _reference(px, py, bd, case["mod"])
    _same(got, ref, name)
    _check_edges(got, px, py, bd, case["mod"], what=name)
    _mir_bound(px, py, bd, case["mod"], case["dtype"], got["scores"], name)
    if case["N"] >= F.PATTERNS:
        rsc = ref[0]
        assert np.isfinite(rsc[3]) and (case["mod"] or np.isfinite(rsc).all()), rsc
        if case["mod"] and case["S"] > 0:
            assert np.isneginf(rsc[6]) and np.isfinite(rsc[5]), rsc


def test_every_bestpath_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- exact ties
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("S", [6, 64])
@pytest.mark.parametrize("mod", [False, True])
def test_ties_on_the_device(dtype, S, mod):
    """Multiples of 0.25: nearly every node is an exact tie, in every storage type the same values.  Then uniform weights: the
    closed forms -- every symbol at t0 (regular), symbol s at t0 + s - s0 (modified)."""
    X, Y, bd = tie_case(S, mod)
    px, py = torch.tensor(X).to(TORCH[dtype]), torch.tensor(Y).to(TORCH[dtype])
    assert np.array_equal(_stored(px), X) and np.array_equal(_stored(py), Y)
    got = call(px.to(DEV), py.to(DEV), bd)
    assert got["st"] == 0
    ref = _reference(px, py, bd, mod)
    assert np.isfinite(ref[0]).all()
    _same(got, ref, "ties")
    _check_edges(got, px, py, bd, mod, what="ties")
    wrong = _reference(px, py, bd, mod, strict=False)               # a library that takes the symbol edge on ties must fail
    assert np.array_equal(wrong[0], ref[0])
    with pytest.raises(AssertionError):
        _same(dict(got, back=ref[2]), (ref[0], wrong[1], ref[2]), "frames of >=")
    with pytest.raises(AssertionError):
        _same(dict(got, frames=ref[1]), (ref[0], ref[1], wrong[2]), "back of >=")
    px, py = torch.full_like(px, -0.5), torch.full_like(py, -0.5)
    got = call(px.to(DEV), py.to(DEV), bd)
    for b, (s0, t0, s1, t1) in enumerate(bd):
        want = np.full(S, -1)
        want[s0:s1] = [t0 + (s - s0 if mod else 0) for s in range(s0, s1)]
        assert np.array_equal(got["frames"][b], want), (b, got["frames"][b])
        assert got["scores"][b] == -0.5 * ((t1 - t0) if mod else (s1 - s0) + (t1 - t0))


# ----------------------------------------------------------------------------- negative control
@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", False), ("f16", True)])
def test_negative_control_another_boundary_is_refused(dtype, mod):
    """The result with one boundary against the reference with another must fail, for scores, frames and back: the checks
    cannot pass on a library that ignores the boundary."""
    N, S, T = 4, 5, 9
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 8], [0, 1, 3, 9], [2, 0, 5, 7]], np.int64)
    other = np.array([[0, 1, 5, 9], [1, 2, 4, 7], [0, 1, 4, 9], [1, 0, 5, 7]], np.int64)
    px, py, bd, mx, my = _problem("neg", dtype, N, S, T, mod, bd, poison_outside=False)
    got = call(px.to(DEV), py.to(DEV), bd)
    assert got["st"] == 0
    ref = _reference(px, py, bd, mod)
    _same(got, ref, "own boundary")
    oth = _reference(px, py, other, mod)
    for i, what in enumerate(("scores", "frames", "back")):
        assert not np.array_equal(ref[i], oth[i]), what                                      # (on the CPU: the references differ)
        mixed = list(ref)
        mixed[i] = oth[i]
        with pytest.raises(AssertionError):
            _same(got, tuple(mixed), "other " + what)


# ----------------------------------------------------------------------------- against this tree
@pytest.mark.parametrize("U", [5, 100])
def test_frames_are_rnnt_aligns_on_planted_logits(U):
    """px, py from log_softmax of planted logits (margin 4): frames equal rnnt_align's; scores agree within COST_TOL["f32"],
    rtol = atol -- the project's cost bound: rnnt_align sums base-2 fp32 terms."""
    from warprnnt_pytorch import rnnt_align
    from warprnnt_pytorch.bestpath import best_path
    from tests.test_gpu_align import planted
    from tests.test_gpu_mi import _from_logits
    rng = np.random.default_rng(U)
    N, T, A = 3, 60, 9
    acts, labels = planted(N, T, U, A, rng, margin=4.0)
    xl = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yl = torch.full((N,), U - 1, dtype=torch.int32, device=DEV)
    score, frames = rnnt_align(acts, labels, xl, yl)
    px, py, bd = _from_logits(acts, labels.cpu().numpy(), np.full(N, T), np.full(N, U - 1), 0, False)
    sc, fr = best_path(px, py, torch.tensor(bd, device=DEV))
    assert torch.equal(fr, frames)
    tol = COST_TOL["f32"]
    print("max |dscore| =", (sc - score).abs().max().item())
    assert torch.allclose(sc, score, rtol=tol, atol=tol), (sc, score)


# ----------------------------------------------------------------------------- call forms and reruns
@pytest.mark.parametrize("dtype,S,mod", [("f32", 8, False), ("bf16", 8, True), ("f32", 65, True), ("f64", 69, False),
                                         ("f16", 1030, False)])
def test_call_forms_agree(dtype, S, mod):
    N, T = 7, 75 if mod else 11
    case = dict(name="forms_%s_%d" % (dtype, S), dtype=dtype, N=N, S=S, T=T, mod=mod)
    px, py, bd, mx, my = _table_problem(case, seed=S)
    xd, yd = px.to(DEV), py.to(DEV)
    for bdx in (bd, None):
        if bdx is None:                              # the full rectangles read everything: no NaN
            px, py, _, mx, my = _problem("full", dtype, N, S, T, mod, None, np.random.default_rng(S))
            xd, yd = px.to(DEV), py.to(DEV)
        one = call(xd, yd, bdx)
        assert one["st"] == 0
        _same(one, _reference(px, py, bdx, mod), "one call")
        _check_edges(one, px, py, bdx, mod, what="one call")
        keys = ("scores", "frames", "back", "ex", "ey")
        same = lambda a, b, ks=keys: all(np.array_equal(a[k], b[k], equal_nan=True) for k in ks)    # noqa: E731
        two, names = profiled(lambda: call(xd, yd, bdx, "noedges"))
        assert two["st"] == 0 and same(one, two, keys[:3])
        seen = stages_seen(names, F.stage_of, F.STAGES)
        assert not names or (seen["sweep"] == F.predict(case)["sweep"] and not seen["edges"]), seen
        host = call(xd, yd, bdx, "host")
        assert host["st"] == 0 and same(one, host)
        e1, names = profiled(lambda: call(xd, yd, bdx, "edges", prev=two))                    # a NULL scale
        assert e1["st"] == 0 and same(one, e1)
        seen = stages_seen(names, F.stage_of, F.STAGES)
        assert not names or (seen["edges"] == F.predict(case)["edges"] and not seen["sweep"]), seen
        scale = 0.5 + 0.25 * np.arange(N)
        scale[1] = -1.5
        e2 = call(xd, yd, bdx, "edges", scale=scale, prev=two)
        assert e2["st"] == 0
        _check_edges(e2, px, py, bdx, mod, scale=scale, what="scaled")
        assert (e2["ex"][1] <= 0).all() and (e2["ey"][1] <= 0).all() and (e2["ey"][1] < 0).any() == np.isfinite(one["scores"][1])
        again = call(xd, yd, bdx)                                                             # a second run: identical bits
        assert again["st"] == 0 and same(one, again)


# ----------------------------------------------------------------------------- the header's edge cases
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("mod", [False, True])
def test_infinite_and_non_finite_edges(dtype, mod):
    """-inf holes with a path around them; no path: -inf, frames -1, zero indicators, the recursion's bits; NaN / +inf on an
    edge of the rectangle: that sample only; a NaN outside every rectangle changes nothing."""
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
    got = call(px.to(DEV), py.to(DEV), bd)
    assert got["st"] == 0
    ref = _reference(px, py, bd, mod)
    rsc = ref[0]
    assert np.isfinite(rsc[0]) and np.isneginf(rsc[1]) and np.isneginf(rsc[2]) == mod and np.isnan(rsc[3:6]).all()
    assert np.isfinite(rsc[6:]).all()
    for b in (3, 4, 5):
        assert np.isnan(got["scores"][b]) and (got["frames"][b] == -1).all(), b
        assert np.isnan(got["ex"][b][mx[b]]).all() and np.isnan(got["ey"][b][my[b]]).all(), b
        assert not got["ex"][b][~mx[b]].any() and not got["ey"][b][~my[b]].any(), b
    keep = [0, 1, 2, 6, 7]
    sub = {k: got[k][keep] for k in ("scores", "frames", "back", "ex", "ey")}
    _same(sub, tuple(r[keep] for r in ref), "limits")                # (no path: the recursion's bits are the reference's)
    _check_edges(sub, px[keep], py[keep], bd[keep], mod, what="limits")
    assert (got["frames"][1] == -1).all() and not got["ex"][1].any() and not got["ey"][1].any()
    again = call(px.to(DEV), py.to(DEV), bd)
    assert np.array_equal(again["back"], got["back"]) and np.array_equal(again["scores"], got["scores"], equal_nan=True)


@pytest.mark.parametrize("mod", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_every_edge_of_the_rectangle_poisons(mod, bad):
    """Sample b carries `bad` on the b-th edge of its rectangle (1, 1, 3, 4) of an S = 3, T = 5 tensor -- every edge of the
    rectangle in turn -- and the last sample none."""
    S, T = 3, 5
    row = (1, 1, 3, 4)
    mx1, my1 = R.edge_masks(1, S, T, mod, np.array([row]))
    ex_idx, ey_idx = np.argwhere(mx1[0]), np.argwhere(my1[0])
    N = len(ex_idx) + len(ey_idx) + 1
    bd = np.tile(np.array(row, np.int64), (N, 1))
    px, py, bd, mx, my = _problem("every", "f32", N, S, T, mod, bd)
    for b, (s, t) in enumerate(ex_idx):
        px[b, s, t] = bad
    for b, (s, t) in enumerate(ey_idx):
        py[len(ex_idx) + b, s, t] = bad
    got = call(px.to(DEV), py.to(DEV), bd)
    again = call(px.to(DEV), py.to(DEV), bd)
    assert got["st"] == 0 and np.array_equal(got["back"], again["back"])
    assert np.isnan(got["scores"][:-1]).all() and (got["frames"][:-1] == -1).all()
    for b in range(N - 1):
        assert np.isnan(got["ex"][b][mx[b]]).all() and np.isnan(got["ey"][b][my[b]]).all(), b
        assert not got["ex"][b][~mx[b]].any() and not got["ey"][b][~my[b]].any(), b
    last = {k: got[k][-1:] for k in ("scores", "frames", "back", "ex", "ey")}
    _same(last, _reference(px[-1:], py[-1:], bd[-1:], mod), "the clean sample")
    assert np.isfinite(last["scores"]).all()


@pytest.mark.parametrize("mod", [False, True])
def test_degenerate_rectangles(mod):
    """fp64.  s1 == s0: the frames alone; t1 == t0: regular the symbols at t0, modified 0 when s1 == s0 and -inf otherwise;
    modified with s1 - s0 == t1 - t0: the diagonal of px; S = 0: px, frames and px_path have no element."""
    N, S, T = 5, 3, 6
    bd = np.array([[2, 1, 2, 5], [0, 4, 3, 4], [1, 3, 1, 3], [0, 2, 3, 5], [0, 0, 3, 6]], np.int64)
    px, py, bd, mx, my = _problem("deg", "f64", N, S, T, mod, bd)
    got = call(px.to(DEV), py.to(DEV), bd)
    assert got["st"] == 0
    _same(got, _reference(px, py, bd, mod), "degenerate")
    _check_edges(got, px, py, bd, mod, what="degenerate")
    sc, fr = got["scores"], got["frames"]
    assert (fr[0] == -1).all() and sc[2] == 0 and (fr[2] == -1).all() and got["ey"][0][my[0]].all()
    if mod:
        assert np.isneginf(sc[1]) and list(fr[3]) == [2, 3, 4] and not got["ey"][3].any()
    else:
        assert list(fr[1]) == [4, 4, 4] and not got["ey"][1].any()
    px0, py0, bd0, mx0, my0 = _problem("s0", "f64", 3, 0, 9, mod, np.array([[0, 0, 0, 9], [0, 3, 0, 4], [0, 5, 0, 5]]))
    for form in ("all", "host", "noedges"):
        got = call(px0.to(DEV), py0.to(DEV), bd0, form)
        assert got["st"] == 0 and got["frames"].size == 0 and not got["back"].any()
        _same(got, _reference(px0, py0, bd0, mod), "S = 0 " + form)
        if form != "noedges":
            assert got["ex"].size == 0 and np.array_equal(got["ey"], my0.astype(np.float64))


def test_invalid_arguments():
    m = _bp()
    lib = m.lib()
    N, S, T = 3, 4, 6
    px, py, bd, mx, my = _problem("inv", "f32", N, S, T, False, poison_outside=False)
    xd, yd = px.to(DEV), py.to(DEV)
    good = call(xd, yd, None)
    assert good["st"] == 0 and np.isfinite(good["scores"]).all()
    # a boundary outside the tensor: the marker -> INVALID_VALUE with host scores; enqueue-only forms mark the sample alone
    for row in ((0, 0, S + 1, T), (0, 0, S, T + 1), (-1, 0, S, T), (0, -1, S, T), (3, 0, 2, T), (0, 5, S, 4),
                (0, 0, 2 ** 40, T), (-2 ** 62, 0, S, T)):
        bad = R.full_boundary(N, S, T)
        bad[1] = row
        for mod in (False, True):
            x2 = xd[:, :, :T].contiguous() if mod else xd
            assert call(x2, yd, bad, "host")["st"] == 2, row
            got = call(x2, yd, bad)
            assert got["st"] == 0 and got["scores"][1:2].view(np.uint64)[0] == 0x7ff8dead00000000, row
            assert (got["frames"][1] == -1).all() and not got["back"][1].any() and not got["ex"][1].any() and not got["ey"][1].any()
            _same(got, _reference(x2.cpu(), py, bad, mod), "bad boundary")
            if not mod:
                for k in ("scores", "frames", "back", "ex", "ey"):
                    assert np.array_equal(got[k][[0, 2]], good[k][[0, 2]]), k
    # NULL pointers; one indicator without the other; dtype codes; the CPU location; sizes; limits; overlaps
    scores = torch.zeros(N, dtype=torch.float64, device=DEV)
    frames = torch.zeros((N, S), dtype=torch.int32, device=DEV)
    back = torch.zeros((N, S + 1, 1), dtype=torch.int64, device=DEV)
    ext, eyt = torch.zeros_like(xd), torch.zeros_like(yd)
    one = lambda **kw: lib.compute_rnnt_bestpath(                                                        # noqa: E731
        kw.get("px", xd.data_ptr()), kw.get("py", yd.data_ptr()), None, kw.get("S", S), kw.get("T", T), kw.get("N", N), 0,
        kw.get("scores", scores.data_ptr()), kw.get("frames", frames.data_ptr()), kw.get("back", back.data_ptr()),
        kw.get("ex", ext.data_ptr()), kw.get("ey", eyt.data_ptr()), kw.get("opt", _opt()), kw.get("code", 0))
    assert one() == 0 and one(ex=None, ey=None) == 0
    assert one(ex=None) == 2 and one(ey=None) == 2
    assert one(px=None) == 2 and one(py=None) == 2 and one(scores=None) == 2 and one(frames=None) == 2 and one(back=None) == 2
    for code in (4, -1):
        assert one(code=code) == 2
    cpu = _opt()
    cpu.loc = 0
    assert one(opt=cpu) == 2
    assert one(S=-1) == 2 and one(T=0) == 2 and one(N=0) == 2
    assert one(ex=yd.data_ptr()) == 2 and one(ey=xd.data_ptr() + 16) == 2 and one(ex=xd.data_ptr()) == 2
    assert one(ex=eyt.data_ptr() + 8) == 2 and one(ex=ext.data_ptr() + 2) == 2 and one(back=scores.data_ptr()) == 2
    assert one(frames=back.data_ptr()) == 2 and one(scores=ext.data_ptr()) == 2 and one(back=back.data_ptr() + 4) == 2
    assert one(S=4096) == 2 and one(S=4095, T=(1 << 13) - 1) == 2 and one(S=15, T=(1 << 12) - 1, N=1 << 16) == 2
    edges = lambda **kw: lib.compute_rnnt_bestpath_edges(                                                # noqa: E731
        kw.get("frames", frames.data_ptr()), kw.get("scores", scores.data_ptr()), None, None, kw.get("S", S), T, N, 0,
        kw.get("ex", ext.data_ptr()), kw.get("ey", eyt.data_ptr()), kw.get("opt", _opt()), kw.get("code", 0))
    assert edges() == 0
    assert edges(frames=None) == 2 and edges(scores=None) == 2 and edges(ex=None) == 2 and edges(ey=None) == 2
    assert edges(code=7) == 2 and edges(opt=cpu) == 2 and edges(S=4096) == 2 and edges(ex=frames.data_ptr()) == 2
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the Python module
def test_python_validation_on_the_device():
    from warprnnt_pytorch.bestpath import best_path
    px, py = torch.zeros(2, 3, 6, device=DEV), torch.zeros(2, 4, 5, device=DEV)
    for row in ((0, 0, 4, 5), (0, 0, 3, 6), (2, 0, 1, 5), (0, -1, 3, 5)):
        bd = torch.tensor([[0, 0, 3, 5], row], device=DEV)
        with pytest.raises(ValueError, match="boundary\\[1\\]"):
            best_path(px, py, bd)
        sc, fr = best_path(px, py, bd, validate=False)          # enqueue only: the library marks the sample
        assert torch.isnan(sc[1]) and torch.isfinite(sc[0]) and (fr[1] == -1).all()
    with pytest.raises(ValueError, match="one device"):
        best_path(px, py, torch.tensor([[0, 0, 3, 5]] * 2))
    with pytest.raises(ValueError, match="px must be"):
        best_path(torch.zeros(2, 3, 7, device=DEV), py)
    for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        sc, fr, (ex, ey), bk = best_path(px.to(dt), py.to(dt), return_edges=True, return_back=True)
        assert sc.dtype == torch.float64 and sc.shape == (2,) and fr.dtype == torch.int32 and fr.shape == (2, 3)
        assert ex.dtype == dt and ex.shape == px.shape and ey.shape == py.shape and bk.shape == (2, 4, 1) and bk.dtype == torch.int64
        assert (fr == 0).all() and (sc == 0).all()
    sc, fr, bk = best_path(px[:, :, :5].contiguous(), py, return_back=True)
    assert fr.tolist() == [[0, 1, 2]] * 2 and len(best_path(px, py)) == 2


@pytest.mark.parametrize("mod", [False, True])
def test_return_edges_and_requires_grad_combinations(mod):
    """return_edges with and without inputs that require grad, and requires grad alone: the same scores and frames bit for
    bit, the reference's indicators, and backward == indicator times grad_output (zero for a sample without a path)."""
    from warprnnt_pytorch.bestpath import best_path
    case = dict(name="rg", dtype="f32", N=7, S=9, T=14, mod=mod)
    px, py, bd, mx, my = _table_problem(case, seed=3)
    xd, yd, bt = px.to(DEV), py.to(DEV), torch.tensor(bd, device=DEV)
    rsc, rfr, rbk = _reference(px, py, bd, mod)
    go = torch.tensor([0.7, -1.3, 2.0, 1.0, 0.25, 3.0, -0.5], dtype=torch.float64, device=DEV)
    ex1, ey1 = R.edges(rfr, rsc, bd, 9, 14, mod)
    wx, wy = R.edges(rfr, rsc, bd, 9, 14, mod, go.cpu().numpy().astype(np.float32).astype(np.float64))
    as32 = lambda a: a.astype(np.float32).astype(np.float64)                                 # noqa: E731
    # 1: return_edges, nothing requires grad
    s1, f1, (gx1, gy1), b1 = best_path(xd, yd, bt, return_edges=True, return_back=True)
    assert not s1.requires_grad and not gx1.requires_grad
    assert np.array_equal(s1.cpu().numpy(), rsc) and np.array_equal(f1.cpu().numpy(), rfr)
    assert np.array_equal(b1.cpu().numpy().view(np.uint64), rbk)
    assert np.array_equal(gx1.double().cpu().numpy(), ex1) and np.array_equal(gy1.double().cpu().numpy(), ey1)
    loss = lambda s: torch.where(torch.isfinite(s), s, torch.zeros_like(s)).mul(go).sum()    # noqa: E731
    # 2: return_edges and requires grad: the indicators once, backward multiplies and launches nothing of the library
    xa, ya = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    s2, f2, (gx2, gy2) = best_path(xa, ya, bt, return_edges=True)
    assert s2.requires_grad and not f2.requires_grad and not gx2.requires_grad and torch.equal(s2.detach(), s1)
    assert torch.equal(gx2, gx1) and torch.equal(gy2, gy1) and torch.equal(f2, f1)
    _, names = profiled(lambda: loss(s2).backward())
    assert not any(F.stage_of(n) is not None for n in names), names
    fin = torch.isfinite(s1).reshape(-1, 1, 1)
    assert np.array_equal(torch.where(fin, xa.grad, torch.zeros_like(xa.grad)).double().cpu().numpy(), as32(wx))
    assert np.array_equal(torch.where(fin, ya.grad, torch.zeros_like(ya.grad)).double().cpu().numpy(), as32(wy))
    # 3: requires grad alone: the edges entry with grad_output as the scale
    xb, yb = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    s3, f3 = best_path(xb, yb, bt)
    assert torch.equal(s3.detach(), s1) and torch.equal(f3, f1)
    _, names = profiled(lambda: loss(s3).backward())
    seen = stages_seen(names, F.stage_of, F.STAGES)
    assert not names or (seen["edges"] == F.predict(case)["edges"] and not seen["sweep"]), seen
    zero = ~np.isfinite(rsc)
    assert zero.any() == mod and not xb.grad[torch.tensor(zero)].any() and not yb.grad[torch.tensor(zero)].any()
    ex3, ey3 = R.edges(rfr, rsc, bd, 9, 14, mod, np.where(zero, 0.0, go.cpu().numpy()))
    assert np.array_equal(xb.grad.double().cpu().numpy(), as32(ex3)) and np.array_equal(yb.grad.double().cpu().numpy(), as32(ey3))


def test_hip_graph_capture_and_replay():
    """Forward + backward captured once (one branch), replayed twice on new inputs."""
    from warprnnt_pytorch.bestpath import best_path
    B, S, T = 3, 5, 9
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 9], [0, 0, 3, 6]], np.int64)
    bt = torch.tensor(bd, device=DEV)
    sx = torch.zeros((B, S, T + 1), device=DEV, requires_grad=True)
    sy = torch.zeros((B, S + 1, T), device=DEV, requires_grad=True)
    _bp().lib()

    def step():
        sx.grad = sy.grad = None
        sc, fr = best_path(sx, sy, bt, validate=False)
        sc.sum().backward()
        return sc, fr

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
        sc, fr = step()
    gxs, gys = sx.grad, sy.grad
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        xn = (rng.standard_normal((B, S, T + 1)) - 1).astype(np.float32)
        yn = (rng.standard_normal((B, S + 1, T)) - 1).astype(np.float32)
        with torch.no_grad():
            sx.copy_(torch.tensor(xn))
            sy.copy_(torch.tensor(yn))
        graph.replay()
        torch.cuda.synchronize()
        rsc, rfr, _ = R.best_path(xn, yn, bd, False)
        ex, ey = R.edges(rfr, rsc, bd, S, T, False)
        assert np.array_equal(sc.detach().cpu().numpy(), rsc) and np.array_equal(fr.cpu().numpy(), rfr)
        assert np.array_equal(gxs.double().cpu().numpy(), ex) and np.array_equal(gys.double().cpu().numpy(), ey)


# ----------------------------------------------------------------------------- long lattices
@pytest.mark.parametrize("S", [300, 32])
def test_long_lattice(S):
    """T = 1500, fp32: five wavefronts and 24 words per row of back (S = 300, the second sample a short rectangle inside) and
    the wave form (S = 32); the traceback stages its rows in two ranges at S = 300."""
    N, T = 2, 1500
    bd = np.array([[0, 0, S, T], [3, 40, min(S, 33), 140]], np.int64)
    px, py, bd, mx, my = _problem("long", "f32", N, S, T, False, bd)
    got = call(px.to(DEV), py.to(DEV), bd)
    assert got["st"] == 0
    ref = _reference(px, py, bd, False)
    assert np.isfinite(ref[0]).all()
    _same(got, ref, "long S = %d" % S)
    _check_edges(got, px, py, bd, False, what="long S = %d" % S)
