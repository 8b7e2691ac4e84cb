"""-m gpu: alignments drawn from the lattice posterior over px / py edge log-probabilities (include/rnnt_sample.h,
libwarprnnt_sample.so).

Every case of tests/sample_forms.py runs through compute_rnnt_sample, then compute_rnnt_path_weights and
compute_rnnt_path_edges on its frames, under torch.profiler: exactly the kernels the release rule predicts run, stage by
stage.  Inputs are NaN outside the rectangles' edge sets (never read); outputs start poisoned (NaN, -7) between 4096 guard
bytes that stay as they were.  The reference (tests/sample_ref.py, numpy fp64) is given the stored values and the case's
uniforms; tests/test_sample_cpu.py has shown that every decision of every case is clear of the device's error in r, so:

    frames              equal to the reference, element for element (-1 outside [s0, s1) and without a path)
    weights             bit-equal to the numpy fp64 loop in walk order over the RETURNED frames (sample_ref.path_weights)
    alpha, scores       |got - ref| <= 1e-9 (1 + |ref|), expect's derived bound; -inf position for position
    entry 2             frames and weights of entry 1, bit for bit
    entry 3             |got - W| <= 2 g sum |w_e|, g = (n - 1) 2^-53 / (1 - (n - 1) 2^-53): two fp64 sums of the same n terms
                        in two orders, each within g sum |w_e| of the exact sum (include/rnnt_sample.h)
    entry 4             integer coeff: every sum is exact in fp64, so fp32 / fp64 storage is bit-equal to the reference and
                        16-bit storage within one rounding, |got - ref| <= u |ref|, u = 2^-8 (bf16), 2^-11 (fp16)

Then: negative controls, the header's edge cases, refusals, `mi` and `bestpath` of this tree as yardsticks, the Python module
with gradcheck, HIP-graph capture and the grid limits."""
import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import sample_forms as F
from tests import sample_ref as R
from tests.gpu_support import CODE, COST_TOL, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, profiled, stages_seen
from tests.test_gpu_bestpath import Guarded

pytestmark = pytest.mark.gpu
NEG = float("-inf")
TOL = COST_TOL["f64"]
MARKER_BITS = 0x7ff8dead00000000
ROUND16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


def _sa():
    from warprnnt_pytorch import sample
    return sample


def _opt(stream=None):
    return G.options(1, 1, 0, stream)                   # (only loc and stream are read)


def _p(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _dims(px, py):
    N, S1, T = py.shape
    return N, S1 - 1, T, int(px.shape[2] == T), CODE[NAME[py.dtype]]


def _bd(bd):
    return None if bd is None else torch.tensor(np.asarray(bd, np.int64), device=DEV)


def sample(px, py, bd, U, stream=None):
    """Entry 1 on device tensors -> dict(st, scores, alpha, frames, weights) as numpy, plus the device tensors alpha_t,
    scores_t for entry 2.  Every output starts as NaN / -7 between guards."""
    N, S, T, mod, code = _dims(px, py)
    K = U.shape[1]
    bt = _bd(bd)
    gs, ga = Guarded((N,), torch.float64, float("nan")), Guarded((N, S + 1, T + 1), torch.float64, float("nan"))
    gf, gw = Guarded((N, K, S), torch.int32, -7), Guarded((N, K), torch.float64, float("nan"))
    st = _sa().lib().compute_rnnt_sample(_p(px), py.data_ptr(), _p(bt), _p(U), S, T, N, K, mod, gs.ptr, ga.ptr, gf.ptr, gw.ptr,
                                         _opt(stream), code)
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in (gs, ga, gf, gw))
    return dict(st=st, scores=gs.t.cpu().numpy(), alpha=ga.t.cpu().numpy(), frames=gf.t.cpu().numpy(), weights=gw.t.cpu().numpy(),
                alpha_t=ga.t, scores_t=gs.t, frames_t=gf.t)


def walk(px, py, bd, alpha_t, scores_t, U):
    """Entry 2 -> dict(st, frames, weights)."""
    N, S, T, mod, code = _dims(px, py)
    K = U.shape[1]
    bt = _bd(bd)
    gf, gw = Guarded((N, K, S), torch.int32, -7), Guarded((N, K), torch.float64, float("nan"))
    st = _sa().lib().compute_rnnt_sample_walk(_p(px), py.data_ptr(), _p(bt), alpha_t.data_ptr(), scores_t.data_ptr(), _p(U), S, T,
                                              N, K, mod, gf.ptr, gw.ptr, _opt(), code)
    torch.cuda.synchronize()
    assert gf.guards_intact() and gw.guards_intact()
    return dict(st=st, frames=gf.t.cpu().numpy(), weights=gw.t.cpu().numpy())


def weights_of(px, py, bd, frames_t):
    """Entry 3 -> (st, weights (B, K))."""
    N, S, T, mod, code = _dims(px, py)
    K = frames_t.shape[1]
    bt = _bd(bd)
    gw = Guarded((N, K), torch.float64, float("nan"))
    st = _sa().lib().compute_rnnt_path_weights(_p(px), py.data_ptr(), _p(bt), _p(frames_t), S, T, N, K, mod, gw.ptr, _opt(), code)
    torch.cuda.synchronize()
    assert gw.guards_intact()
    return st, gw.t.cpu().numpy()


def edges_of(frames_t, coeff, bd, N, S, T, mod, dtype, stream=None):
    """Entry 4 -> (st, px_acc, py_acc) as float64 numpy."""
    K = frames_t.shape[1]
    bt = _bd(bd)
    ct = None if coeff is None else torch.tensor(np.asarray(coeff, np.float64), device=DEV)
    gx = Guarded((N, S, T if mod else T + 1), TORCH[dtype], float("nan"))
    gy = Guarded((N, S + 1, T), TORCH[dtype], float("nan"))
    st = _sa().lib().compute_rnnt_path_edges(_p(frames_t), _p(ct), _p(bt), S, T, N, K, int(mod), gx.ptr, gy.ptr, _opt(stream),
                                             CODE[dtype])
    torch.cuda.synchronize()
    assert gx.guards_intact() and gy.guards_intact()
    return st, gx.t.double().cpu().numpy(), gy.t.double().cpu().numpy()


def _stored(t):
    return t.double().cpu().numpy()


def _check_sweep(got, ref, what=""):
    """scores and alpha against the reference at 1e-9 (1 + |ref|); -inf, the marker and NaN position for position."""
    rs = ref["scores"]
    assert np.array_equal(got["scores"].view(np.uint64) == MARKER_BITS, rs.view(np.uint64) == MARKER_BITS), (what, "marker")
    assert np.array_equal(np.isnan(got["scores"]), np.isnan(rs)), (what, got["scores"], rs)
    assert np.array_equal(np.isneginf(got["scores"]), np.isneginf(rs)), (what, got["scores"], rs)
    fin = np.isfinite(rs)
    err = np.abs(got["scores"][fin] - rs[fin])
    assert (err <= TOL * (1 + np.abs(rs[fin]))).all(), (what, "scores", got["scores"], rs)
    worst = float((err / (TOL * (1 + np.abs(rs[fin])))).max(initial=0))
    for b in range(len(rs)):
        if np.isnan(rs[b]) and rs[b:b + 1].view(np.uint64)[0] != MARKER_BITS:
            continue                                     # NaN or +inf weights: alpha is unspecified
        ga, ra = got["alpha"][b], ref["alpha"][b]
        inf = np.isneginf(ra)
        assert np.array_equal(np.isneginf(ga), inf), (what, b, "alpha: -inf")
        err, bound = np.abs(ga[~inf] - ra[~inf]), TOL * (1 + np.abs(ra[~inf]))
        assert (err <= bound).all(), (what, b, "alpha", float(err.max(initial=0)))
        worst = max(worst, float((err / bound).max(initial=0)))
    print(what, "sweep: worst error / bound = %.3e" % worst)


def _check_walks(got, ref, px, py, bd, mod, what=""):
    """frames against the reference's, weights against the fp64 loop over the returned frames: bit for bit."""
    assert np.array_equal(got["frames"], ref["frames"]), (what, "frames", np.argwhere(got["frames"] != ref["frames"])[:5])
    W, n, sa = R.path_weights(_stored(px), _stored(py), got["frames"], bd, mod)
    rs = ref["scores"]
    for b in range(len(rs)):
        if np.isfinite(rs[b]):
            assert np.array_equal(got["weights"][b], W[b]), (what, b, "weights", got["weights"][b], W[b])
            assert np.array_equal(got["weights"][b], ref["weights"][b]), (what, b)
        elif np.isneginf(rs[b]):
            assert np.isneginf(got["weights"][b]).all() and (got["frames"][b] == -1).all(), (what, b)
        else:
            assert np.isnan(got["weights"][b]).all() and (got["frames"][b] == -1).all(), (what, b)
    return W, n, sa


def _check_path_weights(w3, W, n, sa, what=""):
    assert np.array_equal(np.isnan(w3), np.isnan(W)), (what, "entry 3: NaN", w3, W)
    assert np.array_equal(np.isneginf(w3), np.isneginf(W)), (what, "entry 3: -inf")
    fin = np.isfinite(W)
    m = np.maximum(n - 1, 0) * 2.0 ** -53
    bound = 2 * m / (1 - m) * sa
    err = np.abs(w3[fin] - W[fin])
    assert (err <= bound[fin]).all(), (what, "entry 3", float(err.max(initial=0)))
    print(what, "entry 3: max error %.3e, its bound there %.3e" % ((err.max(), bound[fin][err.argmax()]) if fin.any() else (0, 0)))


def _check_edges(got, ref, dtype, what=""):
    if dtype in ROUND16:
        assert (np.abs(got - ref) <= ROUND16[dtype] * np.abs(ref)).all(), (what, float(np.abs(got - ref).max()))
    else:
        assert np.array_equal(got, ref), (what, np.argwhere(got != ref)[:5])


def _coeff(N, K, seed):
    return np.random.default_rng(seed).integers(-3, 4, (N, K)).astype(np.float64)


# ----------------------------------------------------------------------------- every form of tests/sample_forms.py
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_sample_form(name):
    case = F.CASES[name]
    N, S, T, mod, K, dtype = case["N"], case["S"], case["T"], case["mod"], case["K"], case["dtype"]
    px, py, bd, mx, my, U = F.problem(case)
    xd, yd, ud = px.to(DEV), py.to(DEV), torch.tensor(U, device=DEV)
    coeff = _coeff(N, K, 1)

    def run():
        one = sample(xd, yd, bd, ud)
        return one, weights_of(xd, yd, bd, one["frames_t"]), edges_of(one["frames_t"], coeff, bd, N, S, T, mod, dtype)

    (got, (st3, w3), (st4, ax, ay)), names = profiled(run)
    if got["st"] == 0 and not names:                 # (a profiler session now and then records no device event at all:
        (got, (st3, w3), (st4, ax, ay)), names = profiled(run)      # one more session, judged as the first would have been)
    assert got["st"] == 0 and st3 == 0 and st4 == 0
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case, G.cus()))
    ref = R.sample(_stored(px), _stored(py), U, bd, mod)
    _check_sweep(got, ref, name)
    W, n, sa = _check_walks(got, ref, px, py, bd, mod, name)
    if N >= F.PATTERNS:
        rsc = ref["scores"]
        assert np.isfinite(rsc[3]) and (mod or np.isfinite(rsc).all()), rsc
        if mod and S > 0:
            assert np.isneginf(rsc[6]) and np.isfinite(rsc[5]), rsc
    # entry 2 on entry 1's alpha: the same walks, bit for bit
    two = walk(xd, yd, bd, got["alpha_t"], got["scores_t"], ud)
    assert two["st"] == 0 and np.array_equal(two["frames"], got["frames"])
    assert np.array_equal(two["weights"], got["weights"], equal_nan=True)
    # entries 3 and 4 on those frames
    _check_path_weights(w3, W, n, sa, name)
    rx, ry = R.path_edges(got["frames"], coeff, bd, S, T, mod)
    _check_edges(ax, rx, dtype, name + " px_acc")
    _check_edges(ay, ry, dtype, name + " py_acc")
    assert not ax[~mx].any() and not ay[~my].any()
    st, bx, by = edges_of(got["frames_t"], coeff, bd, N, S, T, mod, dtype)
    assert st == 0 and np.array_equal(ax, bx) and np.array_equal(ay, by)


def test_every_sample_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- negative controls
@pytest.mark.parametrize("name", ["f16_reg_k64", "f32_mod_k65", "bf16_mod_k130"])
def test_negative_control_other_uniforms_give_other_frames(name):
    case = F.CASES[name]
    assert case["K"] >= 64
    px, py, bd, mx, my, U = F.problem(case)
    other = F.uniforms(dict(case, seed=case["seed"] + 1))
    xd, yd = px.to(DEV), py.to(DEV)
    a, b = sample(xd, yd, bd, torch.tensor(U, device=DEV)), sample(xd, yd, bd, torch.tensor(other, device=DEV))
    assert a["st"] == 0 and b["st"] == 0
    assert (a["frames"] != b["frames"]).any(axis=2).any()
    assert np.array_equal(a["alpha"], b["alpha"], equal_nan=True) and np.array_equal(a["scores"], b["scores"], equal_nan=True)
    ref = R.sample(_stored(px), _stored(py), other, bd, case["mod"])
    with pytest.raises(AssertionError):
        _check_walks(a, ref, px, py, bd, case["mod"], "other uniforms")
    _check_walks(b, ref, px, py, bd, case["mod"], "own uniforms")


@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", False), ("f16", True)])
def test_negative_control_another_boundary_is_refused(dtype, mod):
    """The result with one boundary against the reference with another must fail the identical checks."""
    N, S, T, K = 4, 5, 9, 6
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 8], [0, 1, 3, 9], [2, 0, 5, 7]], np.int64)
    other = np.array([[0, 1, 5, 9], [1, 2, 4, 7], [0, 1, 4, 9], [1, 0, 5, 7]], np.int64)
    rng = np.random.default_rng(3)
    px = torch.tensor(rng.standard_normal((N, S, T if mod else T + 1)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    U = rng.random((N, K, S + T), dtype=np.float32)
    got = sample(px.to(DEV), py.to(DEV), bd, torch.tensor(U, device=DEV))
    own, oth = R.sample(_stored(px), _stored(py), U, bd, mod), R.sample(_stored(px), _stored(py), U, other, mod)
    _check_sweep(got, own, "own boundary")
    _check_walks(got, own, px, py, bd, mod, "own boundary")
    with pytest.raises(AssertionError):
        _check_sweep(got, oth, "another boundary")
    with pytest.raises(AssertionError):
        _check_walks(got, oth, px, py, other, mod, "another boundary")


# ----------------------------------------------------------------------------- the header's edge cases
def _edge_problem(dtype, mod, seed=7):
    N, S, T, K = 8, 4, 7, 5
    bd = R.full_boundary(N, S, T)
    bd[3] = (1, 1, 3, 6)
    bd[6] = (0, 2, 4, 7)
    rng = np.random.default_rng(seed)
    px = torch.tensor(rng.standard_normal((N, S, T if mod else T + 1)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    return px, py, bd, rng.random((N, K, S + T), dtype=np.float32)


def _run_and_check(px, py, bd, U, mod, what):
    xd, yd = px.to(DEV), py.to(DEV)
    got = sample(xd, yd, bd, torch.tensor(U, device=DEV))
    assert got["st"] == 0
    ref = R.sample(_stored(px), _stored(py), U, bd, mod)
    for b in range(len(ref["gap"])):
        assert ref["gap"][b] > R.margin(px.shape[1] + py.shape[2] + 1, ref["amax"][b]), (what, b, "pick another seed")
    _check_sweep(got, ref, what)
    W, n, sa = _check_walks(got, ref, px, py, bd, mod, what)
    st, w3 = weights_of(xd, yd, bd, got["frames_t"])
    assert st == 0
    _check_path_weights(w3, W, n, sa, what)
    return got, ref, w3


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("mod", [False, True])
def test_no_path_and_infinite_edges(dtype, mod):
    """-inf holes with a path around them: no walk crosses one; no path: score -inf, frames -1, weights -inf."""
    px, py, bd, U = _edge_problem(dtype, mod)
    T = py.shape[2]
    px[0, 1, 2] = NEG
    py[0, 2, 3] = NEG
    py[0, 0, 0] = NEG
    if not mod:
        px[0, :, T] = NEG                               # k2's own -inf column
    px[1, 2, :] = NEG                                   # symbol 2 can never be emitted: no path
    got, ref, w3 = _run_and_check(px, py, bd, U, mod, "holes")
    assert np.isfinite(got["scores"][0]) and np.isfinite(got["weights"][0]).all() and np.isneginf(got["scores"][1])
    assert (got["frames"][1] == -1).all() and np.isneginf(got["weights"][1]).all()
    N, S, K = got["frames"].shape[0], got["frames"].shape[2], got["frames"].shape[1]
    st, ax, ay = edges_of(got["frames_t"], None, bd, N, S, T, mod, dtype)
    assert st == 0 and not ax[1].any() and not ay[1].any() and np.isnan(w3[1]).all()
    assert ax[0].sum() == K * S


@pytest.mark.parametrize("mod", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_weight_poisons_its_sample_alone(mod, bad):
    px, py, bd, U = _edge_problem("f32", mod)
    clean = sample(px.to(DEV), py.to(DEV), bd, torch.tensor(U, device=DEV))
    px[3, 1, 3] = bad                                   # inside sample 3's rectangle
    py[4, 4, 6] = bad
    px[5, 0, 0] = bad
    py[6, 0, 0] = bad                                   # outside sample 6's rectangle (t0 = 2): nothing changes
    got, ref, _ = _run_and_check(px, py, bd, U, mod, "poisoned")
    for b in (3, 4, 5):
        assert np.isnan(got["scores"][b]) and (got["frames"][b] == -1).all() and np.isnan(got["weights"][b]).all()
    for b in (0, 1, 2, 6, 7):
        for k in ("scores", "alpha", "frames", "weights"):
            assert np.array_equal(got[k][b], clean[k][b]), (k, b)


@pytest.mark.parametrize("mod", [False, True])
def test_degenerate_rectangles(mod):
    """fp64.  s1 == s0: the frames alone; t1 == t0: regular the symbols at t0, modified no path unless s1 == s0; modified
    with s1 - s0 == t1 - t0: the diagonal of px; S = 0: px, frames and the uniforms are not looked at."""
    N, S, T, K = 5, 3, 6, 4
    bd = np.array([[2, 1, 2, 5], [0, 4, 3, 4], [1, 3, 1, 3], [0, 2, 3, 5], [0, 0, 3, 6]], np.int64)
    rng = np.random.default_rng(12)
    px = torch.tensor(rng.standard_normal((N, S, T if mod else T + 1)) - 1.5, dtype=torch.float64)
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float64)
    mx, my = R.edge_masks(N, S, T, mod, bd)
    px[torch.tensor(~mx)] = float("nan")
    py[torch.tensor(~my)] = float("nan")
    U = rng.random((N, K, S + T), dtype=np.float32)
    got, ref, w3 = _run_and_check(px, py, bd, U, mod, "degenerate")
    X, Y = _stored(px), _stored(py)
    assert (got["frames"][0] == -1).all() and np.allclose(got["weights"][0], Y[0, 2, 1:5].sum(), rtol=1e-12, atol=1e-13)
    assert got["scores"][2] == 0 and (got["weights"][2] == 0).all() and (w3[2] == 0).all()
    if mod:
        assert np.isneginf(got["scores"][1]) and (got["frames"][3] == [2, 3, 4]).all()
        assert np.allclose(got["weights"][3], sum(X[3, i, 2 + i] for i in range(3)), rtol=1e-12, atol=1e-13)
    else:
        assert (got["frames"][1] == 4).all() and np.allclose(got["weights"][1], X[1, :, 4].sum(), rtol=1e-12, atol=1e-13)
    bd0 = np.array([[0, 0, 0, 9], [0, 3, 0, 4], [0, 5, 0, 5]])
    py0 = torch.tensor(rng.standard_normal((3, 1, 9)) - 1.5, dtype=torch.float64)
    px0 = torch.zeros((3, 0, 9 if mod else 10), dtype=torch.float64)
    got, ref, w3 = _run_and_check(px0, py0, bd0, np.zeros((3, K, 9), np.float32), mod, "S = 0")
    assert got["frames"].size == 0 and got["weights"][2, 0] == 0 and got["weights"][1, 0] == py0[1, 0, 3].item()
    st, ax, ay = edges_of(torch.zeros((3, K, 0), dtype=torch.int32, device=DEV), None, bd0, 3, 0, 9, mod, "f64")
    assert st == 0 and ax.size == 0 and np.array_equal(ay, K * R.edge_masks(3, 0, 9, mod, bd0)[1].astype(np.float64))


@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", True), ("f16", False)])
def test_rows_of_frames_that_are_no_path(dtype, mod):
    """Entries 3 and 4: a -1 inside [s0, s1), a decreasing row, a value outside [t0, t1], a tie (modified), a bad boundary:
    weight NaN, nothing added, the coefficient never looked at; the legal rows beside them are unaffected."""
    N, S, T = 3, 4, 8
    bd = np.array([[0, 0, 4, 8], [1, 2, 3, 7], [0, 0, 5, 8]], np.int64)     # sample 2: outside the tensor
    good = [0, 2, 3, 7] if mod else [0, 2, 2, 8]
    rows0 = [good, [0, -1, 3, 7], [3, 2, 4, 7], [0, 2, 3, 9 if not mod else 8], [0, 2, 2, 5] if mod else [0, 2, 2, 7], good]
    rows1 = [[-1, 2, 4, -1], [-5, 1, 4, 99], [-1, 4, 2, -1], [-1, 2, 7 if mod else 8, -1], [-1, -1, -1, -1], [9, 3, 6, 9]]
    frames = np.array([rows0, rows1, [good] * 6], np.int32)
    K = frames.shape[1]
    rng = np.random.default_rng(5)
    px = torch.tensor(rng.standard_normal((N, S, T if mod else T + 1)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float32).to(TORCH[dtype])
    coeff = _coeff(N, K, 2)
    coeff[0, 1] = np.nan                                 # on a row that is no path: never looked at
    coeff[1, 2] = np.inf
    ft = torch.tensor(frames, device=DEV)
    st, w3 = weights_of(px.to(DEV), py.to(DEV), bd, ft)
    W, n, sa = R.path_weights(_stored(px), _stored(py), frames, bd, mod)
    want_nan = np.array([[0, 1, 1, 1, 0 if not mod else 1, 0], [0, 1, 1, 1, 1, 0], [1] * 6], bool)
    assert np.array_equal(np.isnan(W), want_nan)
    assert st == 0
    _check_path_weights(w3, W, n, sa, "no path")
    st, ax, ay = edges_of(ft, coeff, bd, N, S, T, mod, dtype)
    rx, ry = R.path_edges(frames, coeff, bd, S, T, mod)
    assert st == 0 and np.isfinite(ax).all() and np.isfinite(ay).all() and not ax[2].any() and not ay[2].any()
    _check_edges(ax, rx, dtype, "no path px_acc")
    _check_edges(ay, ry, dtype, "no path py_acc")


def test_invalid_arguments_and_limits():
    """A boundary outside the tensor: the marker, alpha -inf, frames -1, weights NaN, the other samples untouched; every
    refusal of the header returns INVALID_VALUE with the outputs untouched."""
    lib = _sa().lib()
    N, S, T, K = 3, 4, 6, 5
    rng = np.random.default_rng(1)
    px = torch.tensor(rng.standard_normal((N, S, T + 1)) - 1.5, dtype=torch.float32)
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float32)
    U = rng.random((N, K, S + T), dtype=np.float32)
    xd, yd, ud = px.to(DEV), py.to(DEV), torch.tensor(U, device=DEV)
    good = sample(xd, yd, None, ud)
    assert good["st"] == 0 and np.isfinite(good["scores"]).all()
    for row in ((0, 0, S + 1, T), (0, 0, S, T + 1), (-1, 0, S, T), (0, -1, S, T), (3, 0, 2, T), (0, 5, S, 4),
                (0, 0, 2 ** 40, T), (-2 ** 62, 0, S, T)):
        bad = R.full_boundary(N, S, T)
        bad[1] = row
        for mod in (False, True):
            x2 = xd[:, :, :T].contiguous() if mod else xd
            got = sample(x2, yd, bad, ud)
            assert got["st"] == 0 and got["scores"][1:2].view(np.uint64)[0] == MARKER_BITS, row
            assert np.isneginf(got["alpha"][1]).all() and (got["frames"][1] == -1).all() and np.isnan(got["weights"][1]).all()
            st, w3 = weights_of(x2, yd, bad, good["frames_t"])
            assert st == 0 and np.isnan(w3[1]).all()
            st, ax, ay = edges_of(good["frames_t"], None, bad, N, S, T, mod, "f32")
            assert st == 0 and not ax[1].any() and not ay[1].any()
            if not mod:
                for k in ("scores", "alpha", "frames", "weights"):
                    assert np.array_equal(got[k][[0, 2]], good[k][[0, 2]]), k
    nan = float("nan")
    scores = torch.full((N,), nan, dtype=torch.float64, device=DEV)
    alpha = torch.full((N, S + 1, T + 1), nan, dtype=torch.float64, device=DEV)
    frames = torch.full((N, K, S), -7, dtype=torch.int32, device=DEV)
    weights = torch.full((N, K), nan, dtype=torch.float64, device=DEV)
    ax, ay = torch.full_like(xd, nan), torch.full_like(yd, nan)
    coeff = torch.ones((N, K), dtype=torch.float64, device=DEV)
    cpu = _opt()
    cpu.loc = 0
    d = dict(px=xd.data_ptr(), py=yd.data_ptr(), bd=None, u=ud.data_ptr(), S=S, T=T, N=N, K=K, scores=scores.data_ptr(),
             alpha=alpha.data_ptr(), frames=frames.data_ptr(), weights=weights.data_ptr(), opt=_opt(), code=0,
             ax=ax.data_ptr(), ay=ay.data_ptr(), coeff=coeff.data_ptr(), gframes=good["frames_t"].data_ptr(),
             galpha=good["alpha_t"].data_ptr(), gscores=good["scores_t"].data_ptr())

    def one(**kw):
        a = dict(d, **kw)
        return lib.compute_rnnt_sample(a["px"], a["py"], a["bd"], a["u"], a["S"], a["T"], a["N"], a["K"], 0, a["scores"], a["alpha"],
                                       a["frames"], a["weights"], a["opt"], a["code"])

    def two(**kw):
        a = dict(d, **kw)
        return lib.compute_rnnt_sample_walk(a["px"], a["py"], a["bd"], a["galpha"], a["gscores"], a["u"], a["S"], a["T"], a["N"],
                                            a["K"], 0, a["frames"], a["weights"], a["opt"], a["code"])

    def three(**kw):
        a = dict(d, **kw)
        return lib.compute_rnnt_path_weights(a["px"], a["py"], a["bd"], a["gframes"], a["S"], a["T"], a["N"], a["K"], 0,
                                             a["weights"], a["opt"], a["code"])

    def four(**kw):
        a = dict(d, **kw)
        return lib.compute_rnnt_path_edges(a["gframes"], a["coeff"], a["bd"], a["S"], a["T"], a["N"], a["K"], 0, a["ax"], a["ay"],
                                           a["opt"], a["code"])

    common = [dict(code=4), dict(code=-1), dict(opt=cpu), dict(S=-1), dict(T=0), dict(N=0), dict(K=0), dict(K=1025), dict(S=1024),
              dict(S=1023, T=(1 << 15) - 1), dict(S=15, T=(1 << 12) - 1, N=1 << 16, K=1), dict(S=1000, T=4, N=4096, K=1024),
              dict(S=0, T=1, N=1 << 22, K=1024)]
    for kw in common + [dict(px=None), dict(py=None), dict(u=None), dict(scores=None), dict(alpha=None), dict(frames=None),
                        dict(weights=None), dict(scores=xd.data_ptr()), dict(alpha=yd.data_ptr()), dict(frames=ud.data_ptr()),
                        dict(weights=alpha.data_ptr() + 8), dict(weights=scores.data_ptr()), dict(scores=scores.data_ptr() + 4),
                        dict(frames=frames.data_ptr() + 2), dict(alpha=alpha.data_ptr() + 4), dict(u=ud.data_ptr() + 2)]:
        assert one(**kw) == 2, kw
    for kw in common + [dict(px=None), dict(py=None), dict(u=None), dict(galpha=None), dict(gscores=None), dict(frames=None),
                        dict(weights=None), dict(weights=d["galpha"]), dict(weights=d["gscores"]), dict(frames=ud.data_ptr()),
                        dict(galpha=d["galpha"] + 4)]:
        assert two(**kw) == 2, kw
    for kw in common + [dict(px=None), dict(py=None), dict(gframes=None), dict(weights=None), dict(weights=d["gframes"]),
                        dict(weights=xd.data_ptr()), dict(weights=weights.data_ptr() + 4), dict(gframes=d["gframes"] + 2)]:
        assert three(**kw) == 2, kw
    for kw in common + [dict(gframes=None), dict(ax=None), dict(ay=None), dict(ax=d["gframes"]), dict(ay=coeff.data_ptr()),
                        dict(ay=ax.data_ptr() + 16), dict(ax=ax.data_ptr() + 2), dict(coeff=coeff.data_ptr() + 4)]:
        assert four(**kw) == 2, kw
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (scores, alpha, weights, ax, ay)) and (frames == -7).all()     # untouched
    assert one() == 0 and two() == 0 and three() == 0 and four() == 0 and four(coeff=None) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- against this tree
@pytest.mark.parametrize("dtype,mod", [("f32", False), ("f64", True), ("bf16", True), ("f16", False)])
def test_scores_are_mi_and_best_path_rescored(dtype, mod):
    """scores against mutual_information_recursion's at COST_TOL[dtype] (the project's tolerance for `mi`); path_scores on
    best_path's frames against best_path's score (the same edges added in another order: entry 3's bound) and its gradient
    against px_path / py_path, bit for bit."""
    from warprnnt_pytorch.bestpath import best_path
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    from warprnnt_pytorch.sample import path_scores, sample_paths
    case = dict(name="mi_%s" % dtype, dtype=dtype, N=7, S=20, T=33, mod=mod, K=4, seed=0)
    px, py, bd, mx, my, U = F.problem(case)
    clean = lambda t: torch.nan_to_num(t, nan=-1.0).to(DEV)                                  # noqa: E731  (autograd adds the tensors)
    xd, yd, bt = clean(px), clean(py), torch.tensor(bd, device=DEV)
    frames, logq, scores = sample_paths(xd, yd, 4, bt, uniforms=torch.tensor(U, device=DEV))
    sc = mir(xd, yd, bt).double().cpu().numpy()
    got = scores.cpu().numpy()
    assert np.array_equal(np.isneginf(sc), np.isneginf(got))
    fin = np.isfinite(got)
    print("max |dscore| =", np.abs(sc[fin] - got[fin]).max())
    assert np.allclose(sc[fin], got[fin], rtol=COST_TOL[dtype], atol=COST_TOL[dtype])
    assert (logq.cpu()[torch.tensor(fin)] <= 1e-9).all()
    xa, ya = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    best, bframes, (ex, ey) = best_path(xa, ya, bt, return_edges=True)
    ws = path_scores(xa, ya, bframes, bt)
    assert ws.shape == (7, 1) and ws.dtype == torch.float64
    bs, w = best.detach().cpu().numpy(), ws.detach().cpu().numpy()[:, 0]
    _, n, sa = R.path_weights(_stored(xd), _stored(yd), bframes.cpu().numpy(), bd, mod)
    has = np.isfinite(bs)
    m = np.maximum(n[:, 0] - 1, 0) * 2.0 ** -53
    assert (np.abs(w[has] - bs[has]) <= (2 * m / (1 - m) * sa[:, 0])[has]).all(), (w, bs)
    assert np.isnan(w[~has]).all() or not (~has).any()          # no path: frames -1 is no path of a rectangle with symbols
    ws[torch.tensor(has)].sum().backward()
    keep = torch.tensor(has, device=DEV)[:, None, None]
    ex, ey = ex.detach(), ey.detach()
    assert torch.equal(xa.grad, torch.where(keep, ex, torch.zeros_like(ex)))
    assert torch.equal(ya.grad, torch.where(keep, ey, torch.zeros_like(ey)))


# ----------------------------------------------------------------------------- the Python module
def test_python_module_on_the_device():
    from warprnnt_pytorch.sample import path_scores, sample_paths
    px, py = torch.zeros(2, 3, 6, device=DEV), torch.zeros(2, 4, 5, device=DEV)
    for row in ((0, 0, 4, 5), (0, 0, 3, 6), (2, 0, 1, 5), (0, -1, 3, 5)):
        bd = torch.tensor([[0, 0, 3, 5], row], device=DEV)
        with pytest.raises(ValueError, match="boundary\\[1\\]"):
            sample_paths(px, py, 4, bd)
        frames, logq, sc = sample_paths(px, py, 4, bd, validate=False)                       # enqueue only: the sample is marked
        assert torch.isnan(sc[1]) and torch.isfinite(sc[0]) and (frames[1] == -1).all() and torch.isnan(logq[1]).all()
    with pytest.raises(ValueError, match="one device"):
        sample_paths(px, py, 4, torch.tensor([[0, 0, 3, 5]] * 2))
    with pytest.raises(ValueError, match="device of px"):
        sample_paths(px, py, 4, uniforms=torch.zeros(2, 4, 8))
    with pytest.raises(ValueError, match="shape"):
        sample_paths(px, py, 4, uniforms=torch.zeros(2, 4, 9, device=DEV))
    with pytest.raises(ValueError, match="num_samples"):
        sample_paths(px, py, 0)
    with pytest.raises(ValueError, match="device of px"):
        path_scores(px, py, torch.zeros(2, 3, dtype=torch.int32))
    g = torch.Generator(device=DEV)
    for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        g.manual_seed(5)
        frames, logq, sc, alpha = sample_paths(px.to(dt), py.to(dt), 64, generator=g, return_alpha=True)
        assert frames.shape == (2, 64, 3) and frames.dtype == torch.int32 and logq.shape == (2, 64) and sc.shape == (2,)
        assert logq.dtype == sc.dtype == alpha.dtype == torch.float64 and alpha.shape == (2, 4, 6)
        assert not logq.requires_grad and torch.allclose(sc, torch.full_like(sc, np.log(56.0)), rtol=1e-12)
        assert torch.allclose(logq, torch.full_like(logq, -np.log(56.0)), rtol=1e-12)        # uniform: 1 / C(8, 3)
        assert len({tuple(r) for r in frames[0].tolist()}) > 20
        g.manual_seed(5)
        again = sample_paths(px.to(dt), py.to(dt), 64, generator=g)
        assert torch.equal(again[0], frames) and torch.equal(again[1], logq)                 # the caller's generator
        assert torch.equal(path_scores(px.to(dt), py.to(dt), frames), torch.zeros_like(logq))
        assert path_scores(px.to(dt), py.to(dt), frames[:, 0].contiguous()).shape == (2, 1)
    mfr, mlogq, msc = sample_paths(px[:, :, :5].contiguous(), py, 8)
    assert (mfr[:, :, 1:] > mfr[:, :, :-1]).all() and torch.allclose(msc, torch.full_like(msc, np.log(10.0)), rtol=1e-12)


@pytest.mark.parametrize("mod", [False, True])
def test_gradcheck_fp64(mod):
    from warprnnt_pytorch.sample import path_scores, sample_paths
    rng = np.random.default_rng(2)
    B, S, T = 3, 2, 4
    mk = lambda shape: torch.tensor(rng.standard_normal(shape) - 1, dtype=torch.float64, device=DEV, requires_grad=True)    # noqa: E731
    px, py = mk((B, S, T if mod else T + 1)), mk((B, S + 1, T))
    bd = torch.tensor([[0, 0, 2, 4], [1, 1, 2, 4], [0, 0, 2, 3]], device=DEV)
    frames = sample_paths(px.detach(), py.detach(), 5, bd)[0]
    frames[2, 4, 0] = 7                                  # a row that is no path: NaN forward, no gradient
    fn = lambda a, b: torch.nan_to_num(path_scores(a, b, frames, bd), nan=0.0)               # noqa: E731
    assert torch.isnan(path_scores(px, py, frames, bd)[2, 4])
    assert torch.autograd.gradcheck(fn, (px, py), eps=1e-6, atol=1e-6, nondet_tol=0.0)


def test_hip_graph_capture_and_replay():
    """Entries 1 and 4 (sample_paths, then path_scores' backward on its frames) captured once on one stream (one branch) with
    validate=False, replayed on new inputs and new uniforms."""
    from warprnnt_pytorch.sample import path_scores, sample_paths
    B, S, T, K = 3, 5, 9, 7
    bd = np.array([[0, 0, 5, 9], [1, 2, 4, 9], [0, 0, 3, 6]], np.int64)
    bt = torch.tensor(bd, device=DEV)
    sx = torch.zeros((B, S, T + 1), device=DEV, requires_grad=True)
    sy = torch.zeros((B, S + 1, T), device=DEV, requires_grad=True)
    su = torch.rand((B, K, S + T), device=DEV)
    go = torch.tensor(_coeff(B, K, 4), device=DEV)
    _sa().lib()

    def step():
        sx.grad = sy.grad = None
        frames, logq, sc = sample_paths(sx, sy, K, bt, uniforms=su, validate=False)
        w = path_scores(sx, sy, frames, bt, validate=False)
        (w * go).sum().backward()
        return frames, logq, sc, w

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
        frames, logq, sc, w = step()
    gx, gy = sx.grad, sy.grad
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        X = (rng.standard_normal(sx.shape) - 1).astype(np.float32)
        Y = (rng.standard_normal(sy.shape) - 1).astype(np.float32)
        U = rng.random(su.shape, dtype=np.float32)
        with torch.no_grad():
            sx.copy_(torch.tensor(X))
            sy.copy_(torch.tensor(Y))
            su.copy_(torch.tensor(U))
        graph.replay()
        torch.cuda.synchronize()
        ref = R.sample(X, Y, U, bd, False)
        assert min(ref["gap"]) > R.margin(S + T + 1, ref["amax"].max())
        got = dict(scores=sc.cpu().numpy(), frames=frames.cpu().numpy(), weights=(logq + sc[:, None]).cpu().numpy())
        assert np.array_equal(got["frames"], ref["frames"])
        assert np.allclose(got["scores"], ref["scores"], rtol=1e-9) and np.allclose(got["weights"], ref["weights"], rtol=1e-9)
        rx, ry = R.path_edges(ref["frames"], go.cpu().numpy(), bd, S, T, False)
        assert np.array_equal(gx.double().cpu().numpy(), rx) and np.array_equal(gy.double().cpu().numpy(), ry)


# ----------------------------------------------------------------------------- the grid limits
@pytest.mark.parametrize("B,K,S,T", [(65536 + 3, 1, 1, 1), (70, 1024, 1, 2)])
def test_grid_limits(B, K, S, T):
    """B past 65535 with one walk, and B K past 65535 with K = 1024 (four walk blocks per sample): every entry against the
    reference."""
    rng = np.random.default_rng(B)
    px = torch.tensor(rng.standard_normal((B, S, T + 1)) - 1.5, dtype=torch.float32)
    py = torch.tensor(rng.standard_normal((B, S + 1, T)) - 1.5, dtype=torch.float32)
    U = rng.random((B, K, S + T), dtype=np.float32)
    xd, yd, ud = px.to(DEV), py.to(DEV), torch.tensor(U, device=DEV)
    got = sample(xd, yd, None, ud)
    assert got["st"] == 0
    # the reference walks sample by sample: every sample where there are few, else the first, the last and 200 drawn ones
    idx = np.arange(B) if B <= 1000 else np.unique(np.concatenate([np.arange(100), np.arange(B - 100, B), rng.integers(0, B, 200)]))
    ref = R.sample(_stored(px)[idx], _stored(py)[idx], U[idx], None, False)
    assert (ref["gap"] > R.margin(S + T + 1, ref["amax"].max())).all()
    _check_sweep({k: got[k][idx] for k in ("scores", "alpha")}, ref, "grid")
    assert np.array_equal(got["frames"][idx], ref["frames"]) and np.array_equal(got["weights"][idx], ref["weights"])
    assert np.isfinite(got["scores"]).all() and np.isfinite(got["weights"]).all()
    assert ((got["frames"] >= 0) & (got["frames"] <= T)).all()
    two = walk(xd, yd, None, got["alpha_t"], got["scores_t"], ud)
    assert two["st"] == 0 and np.array_equal(two["frames"], got["frames"]) and np.array_equal(two["weights"], got["weights"])
    st, w3 = weights_of(xd, yd, None, got["frames_t"])
    # S = 1, T <= 2: at most 3 edges, summed in another order
    assert st == 0 and np.allclose(w3, got["weights"], rtol=0, atol=2 * 2 * 2.0 ** -53 * np.abs(_stored(px)).max() * 3)
    coeff = _coeff(B, K, 6)
    st, ax, ay = edges_of(got["frames_t"], coeff, None, B, S, T, False, "f32")
    fr = got["frames"][:, :, 0]                          # (B, K): the t of the one symbol edge
    rx = np.stack([(coeff * (fr == t)).sum(1) for t in range(T + 1)], axis=1)[:, None, :]
    ry0 = np.stack([(coeff * (fr > t)).sum(1) for t in range(T)], axis=1)
    ry1 = np.stack([(coeff * (fr <= t)).sum(1) for t in range(T)], axis=1)
    assert st == 0 and np.array_equal(ax, rx) and np.array_equal(ay, np.stack([ry0, ry1], axis=1))
