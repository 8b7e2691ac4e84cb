"""-m gpu: best-path alignment (compute_rnnt_align / compute_rnnt_align_add through warprnnt_pytorch) against an fp64 Viterbi
of the fp64 log_softmax of the STORED activations, with the tie rule of include/rnnt.h (blank predecessor on an exact tie).
One case per row-statistics form of tests/kernel_forms.py feeds the aligner, plus the c2, c3 and c4 shapes of bench.py."""
import zlib

import numpy as np
import pytest
import torch

from tests import kernel_forms as K
from warprnnt_pytorch import rnnt_align, rnnt_loss
from warprnnt_pytorch.add_network import rnnt_align_add

pytestmark = pytest.mark.gpu

_TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}
DEV = "cuda:0"


# ----------------------------------------------------------------------------- fp64 reference
def lattice_terms(acts, labels, blank):
    """(N,T,U) fp64 numpy arrays of log p(blank) and log p(label u) from the stored activations (one sample at a time)."""
    N, T, U, A = acts.shape
    pb = np.empty((N, T, U))
    pl = np.full((N, T, U), -np.inf)
    for b in range(N):
        x = acts[b].double()
        lse = torch.logsumexp(x, -1)
        pb[b] = (x[..., blank] - lse).cpu().numpy()
        if U > 1:
            lab = labels[b].long().view(1, U - 1, 1).expand(T, U - 1, 1)
            pl[b, :, :U - 1] = (x[:, :U - 1].gather(-1, lab).squeeze(-1) - lse[:, :U - 1]).cpu().numpy()
    return pb, pl


def viterbi(pb, pl, T, U):
    """One sample, U labels, vectorised over the anti-diagonals.  Returns (score, frames[U]) with the strict tie rule."""
    NEG = -np.inf
    if np.isnan(pb[:T, :U + 1]).any() or np.isnan(pl[:T, :U]).any():
        return float("nan"), [-1] * U
    D = T + U
    diag = [None] * D                                # diag[n][u] = best prefix score of cell (n - u, u)
    a = np.full(U + 1, NEG)
    a[0] = 0.0
    diag[0] = a
    us = np.arange(U + 1)
    for n in range(1, D):
        t = n - us
        prev = diag[n - 1]
        tb = t - 1                                    # blank predecessor (t-1, u), on diagonal n-1 at u
        ok_b = (tb >= 0) & (tb < T)
        stay = np.where(ok_b, prev + pb[np.clip(tb, 0, T - 1), us], NEG)
        ok_l = (us >= 1) & (t >= 0) & (t < T)         # label predecessor (t, u-1), on diagonal n-1 at u-1
        emit = np.full(U + 1, NEG)
        emit[1:] = np.where(ok_l[1:], prev[:-1] + pl[np.clip(t[1:], 0, T - 1), us[:-1]], NEG)
        cell = (t >= 0) & (t < T)
        diag[n] = np.where(cell, np.where(emit > stay, emit, stay), NEG)
    s = diag[D - 1][U] + pb[T - 1, U]
    if not np.isfinite(s):
        return s, [-1] * U
    frames = [-1] * U
    t, u = T - 1, U
    while t > 0 or u > 0:
        n = t + u
        label = u > 0 and (t == 0 or diag[n - 1][u - 1] + pl[t, u - 1] > diag[n - 1][u] + pb[t - 1, u])
        if label:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return s, frames


def rescore(pb, pl, T, U, frames):
    s, u = 0.0, 0
    for t in range(T):
        while u < U and frames[u] == t:
            s += pl[t, u]
            u += 1
        s += pb[t, u]
    return s


def check(acts, labels, xl, yl, blank, score, frames, exact=False):
    pb, pl = lattice_terms(acts, labels, blank)
    score, frames = score.cpu().numpy(), frames.cpu().numpy()
    xl, yl = xl.cpu().numpy(), yl.cpu().numpy()
    for b in range(acts.shape[0]):
        T, U = int(xl[b]), int(yl[b])
        s, fr = viterbi(pb[b], pl[b], T, U)
        f = [int(v) for v in frames[b, :U]]
        assert (frames[b, U:] == -1).all(), b
        if not np.isfinite(s):
            assert (np.isnan(s) and np.isnan(score[b])) or score[b] == s, (b, score[b], s)
            assert (frames[b] == -1).all(), b
            continue
        tol = 1e-4 * max(1.0, abs(s))
        assert abs(score[b] - s) <= tol, (b, score[b], s)
        # a valid path: non-decreasing frames inside [0, T-1], rescored in fp64 within the bound of the optimum
        assert all(0 <= v < T for v in f) and all(f[i] <= f[i + 1] for i in range(U - 1)), (b, f)
        assert abs(rescore(pb[b], pl[b], T, U, f) - s) <= tol, b
        if exact:
            assert f == fr, (b, f, fr)


def inputs(N, T, U, A, dtype, rng, blank=0, ragged=True):
    acts = torch.tensor(rng.standard_normal((N, T, U, A)).astype(np.float32), device=DEV).to(dtype)
    labels = torch.tensor(rng.integers(1, A, size=(N, U - 1)) if A > 1 else np.zeros((N, U - 1)), dtype=torch.int32, device=DEV)
    if blank != 0 and A > 1:
        labels[labels == blank] = 0
    xl = np.full(N, T, np.int32)
    yl = np.full(N, U - 1, np.int32)
    if ragged and N > 1:
        xl[1:] = rng.integers(1, T + 1, size=N - 1)
        yl[1:] = rng.integers(0, U, size=N - 1)
    return acts, labels, torch.tensor(xl, device=DEV), torch.tensor(yl, device=DEV)


def planted(N, T, U, A, rng, margin=4.0):
    """Logits whose best path beats every other by >= 1 nat per decision: a random monotone path gets +margin on the
    symbol it takes at each of its cells."""
    acts = torch.zeros((N, T, U, A))
    labels = torch.tensor(rng.integers(1, A, size=(N, U - 1)), dtype=torch.int32)
    for b in range(N):
        fr = np.sort(rng.integers(0, T, size=U - 1))
        u = 0
        for t in range(T):
            while u < U - 1 and fr[u] == t:
                acts[b, t, u, labels[b, u]] = margin
                u += 1
            acts[b, t, u, 0] = margin
    return acts.to(DEV), labels.to(DEV)


# ----------------------------------------------------------------------------- one case per statistics form
def _stats_cases():
    seen, out = set(), []
    cus = 256
    for name, c in K.CASES.items():
        if c.get("layout") == "packed":
            continue
        n, T, U, A = K.case_shape(c, cus)
        if n * T * U * A > (1 << 26):
            continue
        form = tuple(sorted(K.predict(dict(c, misalign=False), cus)["stats"]))
        if form not in seen:
            seen.add(form)
            out.append(name)
    return out


@pytest.mark.parametrize("name", _stats_cases())
def test_align_every_stats_form(name):
    case = K.CASES[name]
    N, T, U, A = K.case_shape(case, torch.cuda.get_device_properties(0).multi_processor_count)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    acts, labels, xl, yl = inputs(N, T, U, A, _TORCH[case["dtype"]], rng)
    score, frames = rnnt_align(acts, labels, xl, yl)
    check(acts, labels, xl, yl, 0, score, frames)


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(4, 20, 9, 11), (2, 40, 130, 7), (2, 9, 301, 5)])
def test_align_dtypes_and_widths(dtype, shape):
    rng = np.random.default_rng(sum(shape))
    acts, labels, xl, yl = inputs(*shape, _TORCH[dtype], rng, blank=2)
    score, frames = rnnt_align(acts, labels, xl, yl, blank=2)
    check(acts, labels, xl, yl, 2, score, frames)
    # the loss on the same inputs: the best path is one of the paths it sums
    cost = rnnt_loss(acts, labels, xl, yl, blank=2, reduction="none").double()
    assert (score <= -cost + 1e-3 * torch.clamp(cost.abs(), min=1)).all()
    # bit-identical on a second run
    s2, f2 = rnnt_align(acts, labels, xl, yl, blank=2)
    assert torch.equal(score, s2) and torch.equal(frames, f2)


@pytest.mark.parametrize("cfg", [(16, 150, 41, 28), (128, 150, 21, 5000), (64, 1500, 301, 50)], ids=["c2", "c3", "c4"])
def test_align_bench_shapes(cfg):
    N, T, U, A = cfg
    rng = np.random.default_rng(N)
    acts = torch.randn((N, T, U, A), device=DEV, generator=torch.Generator(DEV).manual_seed(N))
    labels = torch.tensor(rng.integers(1, A, size=(N, U - 1)), dtype=torch.int32, device=DEV)
    xl = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yl = torch.full((N,), U - 1, dtype=torch.int32, device=DEV)
    score, frames = rnnt_align(acts, labels, xl, yl)
    check(acts[:4], labels[:4], xl[:4], yl[:4], 0, score[:4], frames[:4])
    cost = rnnt_loss(acts, labels, xl, yl, reduction="none").double()
    assert (score <= -cost + 1e-3 * torch.clamp(cost.abs(), min=1)).all()


@pytest.mark.parametrize("U", [5, 100, 301])
def test_align_planted_exact(U):
    rng = np.random.default_rng(U)
    N, T, A = 3, 60, 9
    acts, labels = planted(N, T, U, A, rng)
    xl = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yl = torch.full((N,), U - 1, dtype=torch.int32, device=DEV)
    for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        x = acts.to(dt)
        score, frames = rnnt_align(x, labels, xl, yl)
        check(x, labels, xl, yl, 0, score, frames, exact=True)


@pytest.mark.parametrize("U", [6, 80])
def test_align_uniform_tie(U):
    N, T, A = 2, 30, 5
    acts = torch.zeros((N, T, U, A), device=DEV)
    labels = torch.full((N, U - 1), 3, dtype=torch.int32, device=DEV)
    xl = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yl = torch.full((N,), U - 1, dtype=torch.int32, device=DEV)
    score, frames = rnnt_align(acts, labels, xl, yl)
    assert (frames == 0).all()
    assert torch.allclose(score.cpu(), torch.full((N,), -(T + U - 1) * np.log(A), dtype=torch.float64))
    sa, fa = rnnt_align_add(torch.zeros((N, T, A), device=DEV), torch.zeros((N, U, A), device=DEV), labels, xl, yl)
    assert (fa == 0).all()


def test_align_non_finite():
    rng = np.random.default_rng(5)
    N, T, U, A = 4, 7, 5, 6
    acts, labels, xl, yl = inputs(N, T, U, A, torch.float32, rng, ragged=False)
    labels[1] = 2
    acts[1, :, :, 0] = -float("inf")                  # no blank anywhere: no finite path
    acts[2, 3, 1, 4] = float("nan")                    # NaN in an in-lattice row
    acts[3, 2, 1, labels[3, 1]] = -float("inf")        # one label cell forbidden: another path wins
    score, frames = rnnt_align(acts, labels, xl, yl)
    s, f = score.cpu(), frames.cpu()
    assert s[1] == -float("inf") and (f[1] == -1).all()
    assert torch.isnan(s[2]) and (f[2] == -1).all()
    assert torch.isfinite(s[0]) and torch.isfinite(s[3])
    check(acts[[0, 3]], labels[[0, 3]], xl[[0, 3]], yl[[0, 3]], 0, score[[0, 3]], frames[[0, 3]])
    # label == blank
    lab0 = torch.zeros_like(labels)
    score, frames = rnnt_align(acts[[0]], lab0[[0]], xl[[0]], yl[[0]])
    check(acts[[0]], lab0[[0]], xl[[0]], yl[[0]], 0, score, frames)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(3, 30, 7, 16), (2, 25, 90, 40)])
def test_align_add_matches_materialised(dtype, shape):
    N, T, U, A = shape
    g = torch.Generator(DEV).manual_seed(U)
    f = torch.randn((N, T, A), device=DEV, generator=g).to(dtype)
    p = torch.randn((N, U, A), device=DEV, generator=g).to(dtype)
    labels = torch.randint(1, A, (N, U - 1), device=DEV, generator=g, dtype=torch.int32)
    xl = torch.tensor([T] + [max(1, T - 3 * i) for i in range(1, N)], dtype=torch.int32, device=DEV)
    yl = torch.tensor([U - 1] + [max(0, U - 1 - 2 * i) for i in range(1, N)], dtype=torch.int32, device=DEV)
    score, frames = rnnt_align_add(f, p, labels, xl, yl)
    joint = (f.float().unsqueeze(2) + p.float().unsqueeze(1))
    check(joint, labels, xl, yl, 0, score, frames)
    sm, fm = rnnt_align(joint, labels, xl, yl)
    assert torch.allclose(score, sm, rtol=1e-4, atol=1e-4)


def test_align_add_planted_exact():
    rng = np.random.default_rng(9)
    N, T, U, A = 2, 40, 12, 8
    # planted logits on the materialised entry; the additive entry against the materialised one on the joint it defines
    fr = [np.sort(rng.integers(0, T, size=U - 1)) for _ in range(N)]
    labels = torch.tensor(rng.integers(1, A, size=(N, U - 1)), dtype=torch.int32)
    acts = torch.zeros((N, T, U, A))
    for b in range(N):
        u = 0
        for t in range(T):
            while u < U - 1 and fr[b][u] == t:
                acts[b, t, u, labels[b, u]] = 6.0
                u += 1
            acts[b, t, u, 0] = 6.0
    x = acts.to(DEV)
    xl = torch.full((N,), T, dtype=torch.int32, device=DEV)
    yl = torch.full((N,), U - 1, dtype=torch.int32, device=DEV)
    g = torch.Generator(DEV).manual_seed(3)
    f = torch.randn((N, T, A), device=DEV, generator=g) * 4
    p = torch.randn((N, U, A), device=DEV, generator=g) * 4
    score, frames = rnnt_align_add(f, p, labels.to(DEV), xl, yl)
    sm, fm = rnnt_align(f.unsqueeze(2) + p.unsqueeze(1), labels.to(DEV), xl, yl)
    assert torch.equal(frames, fm)
    assert torch.allclose(score, sm, rtol=1e-5, atol=1e-5)
    s2, f2 = rnnt_align(x, labels.to(DEV), xl, yl)
    check(x, labels.to(DEV), xl, yl, 0, s2, f2, exact=True)


def test_align_enqueues_on_side_stream_without_sync():
    rng = np.random.default_rng(2)
    acts, labels, xl, yl = inputs(4, 200, 41, 30, torch.float32, rng)
    ref_s, ref_f = rnnt_align(acts, labels, xl, yl)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        score, frames = rnnt_align(acts, labels, xl, yl)
        done = torch.cuda.Event()
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    assert torch.equal(score, ref_s) and torch.equal(frames, ref_f)
