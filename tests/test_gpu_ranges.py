"""-m gpu: libwarprnnt_ranges.so (include/rnnt_ranges.h) through warprnnt_pytorch.ranges against tests/ranges_ref.py: `ranges`
element for element, `kept` bit for bit, no tolerance.  The shapes are the smallest that reach every tile width of the
kernels (tests/ranges_ref.py tile(): 32 frames up to S + 1 = 191, then 16, 8, 4, 2, 1), frames one below / at / above the
tile, window widths 1, 2, 5 and S + 1, both slopes, both types, the four storage types, ragged boundaries with NaN outside
the rectangle, and the edge cases the header lists.  A library that is not built is an error, not a skip."""
import numpy as np
import pytest
import torch

from tests import pruned_ref
from tests import ranges_ref as R
from tests.gpu_support import DEV, TORCH

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f64", "bf16", "f16")


def _rg():
    from warprnnt_pytorch import ranges
    ranges.lib()                                           # ImportError when the library is missing
    return ranges


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Bit for bit; a NaN matches a NaN (its payload is nobody's definition)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def _boundary(kind, S, T, R, rng):
    """None, or four ragged rows: the full rectangle, T_b = 1, S_b = 0, S_b < R - 1 (where R allows)."""
    if kind == "none":
        return None
    rows = [[0, 0, S, T], [0, 0, int(rng.integers(0, S + 1)), 1], [0, 0, 0, int(rng.integers(1, T + 1))],
            [0, 0, max(0, min(S, R - 2)), T]]
    return np.array(rows, np.int64)


def _problem(dtype, mod, S, T, bd, rng, B=2):
    """Occupation-like values of the storage type (peaked, non-negative; 16-bit rounding makes ties), NaN wherever the
    header says nothing is read.  Returns the device tensors and the stored values as fp64 numpy."""
    B = B if bd is None else bd.shape[0]
    TX = T if mod else T + 1
    px = torch.tensor(rng.random((B, S, TX)) ** 4, dtype=torch.float32).to(TORCH[dtype])
    py = torch.tensor(rng.random((B, S + 1, T)) ** 4, dtype=torch.float32).to(TORCH[dtype])
    Sbs, Tbs = R.lengths(bd, B, S, T)
    for b in range(B):
        px[b, Sbs[b]:, :] = float("nan")
        px[b, :, Tbs[b]:] = float("nan")                   # (the regular type's column T included)
        py[b, Sbs[b] + 1:, :] = float("nan")
        py[b, :, Tbs[b]:] = float("nan")
    return px.to(DEV), py.to(DEV), px.double().numpy(), py.double().numpy()


def _check(px, py, X, Y, bd, R_, step, what):
    """Both entries against the reference: ranges of entry 1, kept on those ranges and on hand-made ones (negative, past
    S_b)."""
    rg = _rg()
    bt = None if bd is None else torch.tensor(bd, device=DEV)
    B, _, T = Y.shape
    got = rg.prune_ranges_from_occupations(px, py, bt, s_range=R_, step=step)
    want = R.prune_ranges(X, Y, bd, R_, step)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, T)
    assert np.array_equal(got.cpu().numpy(), want), (what, got.cpu().numpy(), want)
    kept = rg.range_coverage(px, py, got, R_, bt)
    assert kept.dtype == torch.float64
    assert _same(kept.cpu().numpy(), R.coverage(X, Y, bd, want, R_)), what
    hand = ((np.arange(B * T).reshape(B, T) * 7) % (Y.shape[1] + 3) - 1).astype(np.int32)
    kept = rg.range_coverage(px, py, torch.tensor(hand, device=DEV), R_, bt)
    assert _same(kept.cpu().numpy(), R.coverage(X, Y, bd, hand, R_)), what
    return want


def _cases(U):
    """Every (T, R, step, boundary) of the grid for S + 1 = U, the storage type and the lattice type rotating through it."""
    S, tf = U - 1, R.tile(U)
    out, k = [], 0
    for T in sorted({1, 3, tf - 1, tf, tf + 1} - {0}):
        for R_ in sorted({r for r in (1, 2, 5, S + 1) if r <= S + 1}):
            for step in sorted({1, max(1, R_ - 1)}):
                for kind in ("none", "ragged"):
                    out.append((DTYPES[k % 4], bool((k // 4) % 2), S, T, R_, step, kind))
                    k += 1
    return out


@pytest.mark.parametrize("U", [1, 2, 63, 64, 65, 130, 192])
def test_ranges_and_coverage_against_the_reference(U):
    """S + 1 in {1, 2, 63, 64, 65, 130} (tile 32) and 192, the first value above the widest tile (tile 16)."""
    assert R.tile(U) == (16 if U == 192 else 32) and R.tile(191) == 32
    rng = np.random.default_rng(U)
    seen, unreachable, lanes = set(), 0, 0
    for dtype, mod, S, T, R_, step, kind in _cases(U):
        bd = _boundary(kind, S, T, R_, rng)
        px, py, X, Y = _problem(dtype, mod, S, T, bd, rng)
        _check(px, py, X, Y, bd, R_, step, (dtype, mod, S, T, R_, step, kind))
        seen.add((dtype, mod))
        smax = max(0, S + 1 - R_)
        unreachable += smax > (T - 1) * step
        lanes += smax > 64
    if U > 2:
        assert len(seen) == 8 and unreachable > 0
    if U == 130:
        assert lanes > 0                                   # more than one start per lane


@pytest.mark.parametrize("dtype,mod,U", [("f32", False, 384), ("bf16", True, 768), ("f64", False, 1536), ("f16", True, 3072),
                                         ("f32", True, 4096)])
def test_the_narrow_tiles(dtype, mod, U):
    """Tiles of 8, 4, 2 and 1 frames: blocks of 256, 256, 128 and 64 threads; the largest S the library takes."""
    S, tf = U - 1, R.tile(U)
    assert tf == {384: 8, 768: 4, 1536: 2, 3072: 1, 4096: 1}[U]
    rng = np.random.default_rng(U)
    for T, R_, step, kind in ((tf + 1, 5, 4, "ragged"), (2 * tf + 1, 5, 1, "none"), (3, S + 1, 1, "none"), (tf, 2, 1, "ragged")):
        bd = _boundary(kind, S, T, R_, rng)
        if bd is not None:
            bd = bd[[0, 1, 3]]
        px, py, X, Y = _problem(dtype, mod, S, T, bd, rng, B=1)
        _check(px, py, X, Y, bd, R_, step, (dtype, mod, S, T, R_, step, kind))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mod", [False, True])
def test_ties_zeros_and_nan(dtype, mod):
    rg = _rg()
    B, S, T, R_ = 2, 9, 7, 3
    TX = T if mod else T + 1
    dt = TORCH[dtype]
    for step in (1, 2):
        # all-equal occupations: every raw start is the smallest; the starts are the repair's alone
        px, py = torch.full((B, S, TX), 0.25, dtype=dt, device=DEV), torch.full((B, S + 1, T), 0.25, dtype=dt, device=DEV)
        got = rg.prune_ranges_from_occupations(px, py, None, R_, step).cpu().numpy()
        smax = S + 1 - R_
        want = R.repair([0] * T, T, S, R_, step)
        assert np.array_equal(got, np.array([want] * B))
        assert want == R.prune_ranges(px.double().cpu().numpy(), py.double().cpu().numpy(), None, R_, step)[0].tolist()
        assert want[0] == 0 and (want[-1] == smax) == (smax <= (T - 1) * step)
        # all-zero occupations, a sample without a path: the same starts, nothing kept
        zx, zy = torch.zeros_like(px), torch.zeros_like(py)
        got0 = rg.prune_ranges_from_occupations(zx, zy, None, R_, step)
        assert np.array_equal(got0.cpu().numpy(), got)
        assert (_bits(rg.range_coverage(zx, zy, got0, R_).cpu().numpy()) == 0).all()
    # a NaN planted in one column: its windows never win there, the other columns are unaffected
    rng = np.random.default_rng(5)
    px, py, X, Y = _problem(dtype, mod, S, T, None, rng)
    clean = _check(px, py, X, Y, None, R_, 2, "clean")
    py[1, 4, 3] = float("nan")
    Y[1, 4, 3] = np.nan
    raw = [R.raw_start(R.column(X, Y, 1, t, S), R_, S)[0] for t in range(T)]
    assert raw[3] not in (2, 3, 4)
    dirty = _check(px, py, X, Y, None, R_, 2, "nan")
    assert np.array_equal(dirty[0], clean[0])
    kept = rg.range_coverage(px, py, torch.tensor(dirty, device=DEV), R_).cpu().numpy()
    assert np.isnan(kept[1, 3]) and np.isfinite(np.delete(kept[1], 3)).all() and np.isfinite(kept[0]).all()
    # every window of a column NaN: the raw start is 0
    py[0, :, 2] = float("nan")
    Y[0, :, 2] = np.nan
    _check(px, py, X, Y, None, R_, 2, "nan column")


def test_a_minibatch_past_the_grid_limit():
    """65536 + 3 samples at T = 2, S = 1: two slices of the grid, every sample against the reference."""
    rg = _rg()
    B, S, T = 65536 + 3, 1, 2
    rng = np.random.default_rng(9)
    X, Y = rng.random((B, S, T + 1), dtype=np.float32), rng.random((B, S + 1, T), dtype=np.float32)
    bd = np.zeros((B, 4), np.int64)
    bd[:, 2], bd[:, 3] = rng.integers(0, S + 1, B), rng.integers(0, T + 1, B)
    px, py, bt = torch.tensor(X, device=DEV), torch.tensor(Y, device=DEV), torch.tensor(bd, device=DEV)
    for R_ in (1, 2):
        got = rg.prune_ranges_from_occupations(px, py, bt, R_, 1)
        kept = rg.range_coverage(px, py, got, R_, bt).cpu().numpy()
        # the reference, vectorised for this shape: S_b in {0, 1}, T_b in {0, 1, 2}
        Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
        Sb, Tb = bd[:, 2], bd[:, 3]
        g0 = Yd[:, 0, :] + np.where(Sb[:, None] > 0, Xd[:, 0, :T], 0.0)
        g1 = Yd[:, 1, :]
        live = np.arange(T)[None, :] < Tb[:, None]
        if R_ == 1:                                        # smax = S_b; T_b = 1 cannot reach smax = 1: s = min(t, smax)
            want = np.where(live & (Sb[:, None] == 1), np.arange(T)[None, :], 0)
            w = np.where(want == 1, 0.0 + g1, 0.0 + g0)
        else:
            want = np.zeros((B, T), np.int64)
            w = np.where(Sb[:, None] == 1, (0.0 + g0) + g1, 0.0 + g0)
        c = np.where(Sb[:, None] == 1, (0.0 + g0) + g1, 0.0 + g0)
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(_bits(kept), _bits(np.where(live, w / c, 0.0)))
        idx = np.concatenate([np.arange(50), np.arange(65500, B)])          # both sides of the slice boundary at 65535
        assert np.array_equal(got.cpu().numpy()[idx], R.prune_ranges(X[idx], Y[idx], bd[idx], R_, 1))
        assert np.array_equal(_bits(kept[idx]), _bits(R.coverage(X[idx], Y[idx], bd[idx], got.cpu().numpy()[idx], R_)))


def test_hip_graph_capture_and_replay():
    """Both entries captured once with validate=False and replayed twice on new occupations: the reference's bits, and the
    same bits from a second replay of the same inputs."""
    rg = _rg()
    B, S, T, R_ = 3, 70, 37, 5
    bd = np.array([[0, 0, 70, 37], [0, 0, 33, 20], [0, 0, 2, 1]], np.int64)
    bt = torch.tensor(bd, device=DEV)
    sx, sy = torch.zeros((B, S, T + 1), device=DEV), torch.zeros((B, S + 1, T), device=DEV)

    def step():
        s = rg.prune_ranges_from_occupations(sx, sy, bt, R_, validate=False)
        return s, rg.range_coverage(sx, sy, s, R_, bt, validate=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        starts, kept = step()
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        X, Y = (rng.random(sx.shape) ** 4).astype(np.float32), (rng.random(sy.shape) ** 4).astype(np.float32)
        sx.copy_(torch.tensor(X))
        sy.copy_(torch.tensor(Y))
        graph.replay()
        torch.cuda.synchronize()
        s1, k1 = starts.cpu().numpy().copy(), kept.cpu().numpy().copy()
        want = R.prune_ranges(X, Y, bd, R_, R_ - 1)
        assert np.array_equal(s1, want) and np.array_equal(_bits(k1), _bits(R.coverage(X, Y, bd, want, R_)))
        starts.fill_(-7)
        kept.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(starts.cpu().numpy(), s1) and np.array_equal(_bits(kept.cpu().numpy()), _bits(k1))


def test_python_module_on_the_device():
    rg = _rg()
    rng = np.random.default_rng(3)
    B, S, T = 2, 6, 9
    for mod in (False, True):
        px, py, X, Y = _problem("f32", mod, S, T, None, rng)
        # the default slope: R - 1 for the regular type, 1 for the modified type; s_range > S is the whole column
        got = rg.prune_ranges_from_occupations(px, py, s_range=3)
        assert np.array_equal(got.cpu().numpy(), R.prune_ranges(X, Y, None, 3, 1 if mod else 2))
        whole = rg.prune_ranges_from_occupations(px, py, s_range=50)
        assert (whole.cpu().numpy() == 0).all() and (rg.range_coverage(px, py, whole, 50).cpu().numpy() == 1.0).all()
        k2 = rg.get_rnnt_prune_ranges(px, py, None, 3)
        assert k2.dtype == torch.int64 and tuple(k2.shape) == (B, T, 3)
        assert np.array_equal(k2.cpu().numpy(), got.cpu().numpy()[..., None] + np.arange(3))
        assert tuple(rg.get_rnnt_prune_ranges(px, py, None, 50).shape) == (B, T, S + 1)
        for bad in (0, 3, 2.0):
            with pytest.raises(ValueError, match="step must be an int"):
                rg.prune_ranges_from_occupations(px, py, s_range=3, step=bad)
        with pytest.raises(ValueError, match="int32 tensor of shape"):
            rg.range_coverage(px, py, got.long(), 3)
        with pytest.raises(ValueError, match="on one device"):
            rg.prune_ranges_from_occupations(px, py, torch.zeros((B, 4), dtype=torch.int64))
        with pytest.raises(ValueError, match="contiguous"):
            rg.range_coverage(px, py, got.t().contiguous().t(), 3)


# ----------------------------------------------------------------------------- end to end
def test_starts_from_mi_occupations_feed_the_pruned_loss():
    """mutual_information_recursion(return_grad=True) of a random lattice -> starts -> rnnt_loss_pruned on random logits:
    finite costs, and the guarantees of the rule."""
    from warprnnt_pytorch.mi import mutual_information_recursion
    from warprnnt_pytorch.pruned import rnnt_loss_pruned
    rg = _rg()
    rng = np.random.default_rng(11)
    B, S, T, R_, A = 4, 9, 14, 4, 7
    Tb, Lb = np.array([14, 9, 14, 5], np.int32), np.array([9, 4, 0, 9], np.int32)
    bd = np.stack([np.zeros(B), np.zeros(B), Lb, Tb], 1).astype(np.int64)
    px = torch.tensor(rng.standard_normal((B, S, T + 1)) - 1.5, dtype=torch.float32, device=DEV)
    py = torch.tensor(rng.standard_normal((B, S + 1, T)) - 1.5, dtype=torch.float32, device=DEV)
    bt = torch.tensor(bd, device=DEV)
    scores, (gx, gy) = mutual_information_recursion(px, py, bt, return_grad=True)
    assert torch.isfinite(scores).all()
    starts = rg.prune_ranges_from_occupations(gx, gy, bt, s_range=R_)
    assert np.array_equal(starts.cpu().numpy(), R.prune_ranges(gx.double().cpu().numpy(), gy.double().cpu().numpy(), bd, R_, R_ - 1))
    s = starts.cpu().numpy()
    for b in range(B):
        assert Lb[b] <= Tb[b] * (R_ - 1)
        assert pruned_ref.check_invariants(s[b], int(Tb[b]), int(Lb[b]), R_) == [], (b, s[b])
        assert (s[b, Tb[b]:] == 0).all()
    kept = rg.range_coverage(gx, gy, starts, R_, bt).cpu().numpy()
    assert ((kept >= 0) & (kept <= 1 + 1e-12)).all() and (kept[0] > 0).all()
    logits = torch.tensor(rng.standard_normal((B, T, R_, A)), dtype=torch.float32, device=DEV, requires_grad=True)
    labels = torch.tensor(rng.integers(1, A, (B, S)), dtype=torch.int32, device=DEV)
    costs = rnnt_loss_pruned(logits, labels, torch.tensor(Tb, device=DEV), torch.tensor(Lb, device=DEV), starts, 0, "none")
    assert torch.isfinite(costs).all() and (costs > 0).all()
    costs.sum().backward()
    assert torch.isfinite(logits.grad).all()


@pytest.mark.parametrize("seed", R.ADD_SEEDS)
def test_mi_occupations_of_an_additive_joint_give_the_ranges_of_prune_ranges(seed):
    """px / py built in fp64 from a random additive joint f + g: the starts from mi's occupations are those of the existing
    prune_ranges(f, g, ...) -- for seeds whose best and runner-up window sums differ by at least 1e-3 relative in every
    frame of the fp64 reference (tests/test_ranges_cpu.py holds the list to that)."""
    from warprnnt_pytorch.mi import mutual_information_recursion
    from warprnnt_pytorch.pruned import prune_ranges
    rg = _rg()
    p = R.additive_problem(seed)
    bt = torch.tensor(p["boundary"], device=DEV)
    px, py = torch.tensor(p["px"], device=DEV), torch.tensor(p["py"], device=DEV)
    _, (gx, gy) = mutual_information_recursion(px, py, bt, return_grad=True)
    got = rg.prune_ranges_from_occupations(gx, gy, bt, s_range=p["R"])
    old = prune_ranges(torch.tensor(p["f"], dtype=torch.float32, device=DEV), torch.tensor(p["g"], dtype=torch.float32, device=DEV),
                       torch.tensor(p["labels"], device=DEV), torch.tensor(p["T_b"], device=DEV),
                       torch.tensor(p["L_b"], device=DEV), p["R"])
    assert np.array_equal(got.cpu().numpy(), old.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), p["ranges"])
