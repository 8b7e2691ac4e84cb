"""-m gpu: the workspace contract of every library (tests/ws_contract.py has the harness and the registry).

test_case, for every case of every library's forms tables and every C-ABI form the library has: the kernels stay inside the
bytes the sizing function returned (guards of 4096 bytes on both sides, the pointer on a 256-byte boundary and 8 bytes past
one); the bits of every output are those of a zero-filled workspace whatever the buffer held -- 0xFF, what the same dims'
failing batch left (which really failed), what a healthy batch of other dims left, what a score-only call left; and _bwd on the
workspace one _fwd left gives, for scales s1, s2, s1, the first result again as the third and a fresh _fwd + _bwd(s2) as the
second.  Bits against bits: no tolerance (the additive joint's float atomics: tests/ws_contract.py, class _Add).

test_autograd_*, for every autograd wrapper at its module's smallest test shape (N = 3, T = 6, U = 4, fp32, reduction
"none"): the same through ctx.workspace -- retain_graph, accumulation, and two graphs of different shapes differentiated in
the reverse order."""
import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import ws_contract as W
from tests.gpu_support import DEV, dev

pytestmark = pytest.mark.gpu


def _short(size_fn):
    return size_fn[len("get_workspace_size_"):] or "main"


CASES = [(fn, name) for fn, lib in W.REGISTRY.items() for name in sorted(lib.cases())]


@pytest.mark.parametrize("size_fn,name", CASES, ids=["%s__%s" % (_short(fn), name) for fn, name in CASES])
def test_case(size_fn, name):
    runs = W.check_case(W.REGISTRY[size_fn], name, G.cus())
    assert runs >= 8                                    # (a library with one form: 3 zero-filled runs, 0xFF, two fills of 2 calls)


@pytest.mark.parametrize("size_fn", sorted(W.REGISTRY))
def test_left_out_cases_stay_covered_on_this_device(size_fn):
    """The leave-out rule with this device's compute-unit count (tests/test_ws_contract_cpu.py holds it at 256)."""
    missing, small = W.uncovered(W.REGISTRY[size_fn], G.cus())
    assert not any(missing.values()) and not small, (missing, small)


# ----------------------------------------------------------------------------- the autograd wrappers
SHAPES = ((3, 6, 4), (4, 9, 6))             # the modules' smallest test shape, and one of other dims
A, H, S = 11, 8, 2


def _lens(N, T, U):
    tl = np.array(([T, T - 1, T - 3] + [T] * N)[:N], np.int32)
    ll = np.array(([U - 1, U - 2, 1] + [U - 1] * N)[:N], np.int32)
    return tl, ll


def _leaf(rng, *shape):
    return torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=DEV).requires_grad_()


def _labels(rng, N, U, lo, hi):
    return rng.integers(lo, hi, size=(N, U - 1)).astype(np.int32)


def _joint(make):
    """A wrapper on one (N, T, U, width) logits tensor: make(N, T, U, rng, tl, ll) -> (width, labels, loss(x, lab, tl, ll))."""
    def build(N, T, U, rng):
        tl, ll = _lens(N, T, U)
        width, labels, loss = make(N, T, U, rng, tl, ll)
        x = _leaf(rng, N, T, U, width)
        lab, ttl, tll = dev(labels, tl, ll)
        return [x], lambda: loss(x, lab, ttl, tll)
    return build


def _rnnt(N, T, U, rng, tl, ll):
    from warprnnt_pytorch import RNNTLoss
    return A, _labels(rng, N, U, 1, A), RNNTLoss(blank=0, reduction="none")


def _hat(N, T, U, rng, tl, ll):
    from warprnnt_pytorch.hat import HATLoss
    return A, _labels(rng, N, U, 0, A - 1), HATLoss(blank=A - 1, reduction="none")


def _tdt(N, T, U, rng, tl, ll):
    from warprnnt_pytorch.tdt import TDTLoss
    durs = (0, 1, 2, 4)
    return A + len(durs), _labels(rng, N, U, 0, A - 1), TDTLoss(durs, blank=A - 1, sigma=0.05, reduction="none")


def _mblank(N, T, U, rng, tl, ll):
    from warprnnt_pytorch.mblank import MultiBlankLoss
    return A, _labels(rng, N, U, 0, A - 3), MultiBlankLoss((2, 4), blank=A - 1, sigma=0.05, reduction="none")


def _mono(N, T, U, rng, tl, ll):
    from warprnnt_pytorch.mono import MonotonicRNNTLoss
    return A, _labels(rng, N, U, 0, A - 1), MonotonicRNNTLoss(blank=A - 1, reduction="none")


def _delay(N, T, U, rng, tl, ll):
    from warprnnt_pytorch.delay import DelayPenalizedRNNTLoss
    return A, _labels(rng, N, U, 0, A - 1), DelayPenalizedRNNTLoss(blank=A - 1, delay_penalty=0.3, reduction="none")


def _ar(N, T, U, rng, tl, ll):
    from tests import ar_ref
    from warprnnt_pytorch.ar import AlignmentRestrictedRNNTLoss
    lo, hi, _ = ar_ref.windows(rng, tl, ll, U)
    tlo, thi = dev(lo, hi)
    loss = AlignmentRestrictedRNNTLoss(blank=A - 1, reduction="none")
    return A, _labels(rng, N, U, 0, A - 1), lambda x, lab, ttl, tll: loss(x, lab, ttl, tll, tlo, thi)


def _kd(N, T, U, rng, tl, ll):
    from warprnnt_pytorch.kd import TransducerKDLoss
    teacher = _leaf(rng, N, T, U, A).detach()
    loss = TransducerKDLoss(A - 1, "collapsed", 2.0, "none")
    return A, _labels(rng, N, U, 0, A), lambda x, lab, ttl, tll: loss(x, teacher, lab, ttl, tll)


def _packed(N, T, U, rng):
    from warprnnt_pytorch.packed import RNNTLossPacked, pack_joint
    tl, ll = _lens(N, T, U)
    lab, ttl, tll = dev(_labels(rng, N, U, 1, A), tl, ll)
    p = pack_joint(_leaf(rng, N, T, U, A).detach(), ttl, tll).contiguous().requires_grad_()
    loss = RNNTLossPacked(blank=0, reduction="none")
    return [p], lambda: loss(p, lab, ttl, tll)


def _add(N, T, U, rng):
    from warprnnt_pytorch.add_network import RNNTLossAdd
    tl, ll = _lens(N, T, U)
    lab, ttl, tll = dev(_labels(rng, N, U, 1, A), tl, ll)
    f, g = _leaf(rng, N, T, A), _leaf(rng, N, U, A)
    loss = RNNTLossAdd(blank=0, reduction="none")
    return [f, g], lambda: loss(f, g, lab, ttl, tll)


def _windows(N, T, U, rng, tl, ll):
    from tests import pruned_ref
    r = np.zeros((N, T), np.int32)
    for b in range(N):
        r[b, :tl[b]] = pruned_ref.ranges_rule(rng.random((tl[b], ll[b] + 1)), int(tl[b]), int(ll[b]), S)
    return r


def _pruned(N, T, U, rng):
    from warprnnt_pytorch.pruned import RNNTLossPruned
    tl, ll = _lens(N, T, U)
    lab, ttl, tll, rg = dev(_labels(rng, N, U, 1, A), tl, ll, _windows(N, T, U, rng, tl, ll))
    x = _leaf(rng, N, T, S, A)
    loss = RNNTLossPruned(blank=0, reduction="none")
    return [x], lambda: loss(x, lab, ttl, tll, rg)


def _pstream(N, T, U, rng):
    from tests import pstream_forms
    from warprnnt_pytorch.pstream import PrunedStreamingRNNTLoss
    tl, ll = _lens(N, T, U)
    s = pstream_forms.ranges(dict(N=N, T=T, U=U, S=S, type=0), tl, ll, rng)
    lab, ttl, tll, rg = dev(_labels(rng, N, U, 0, A - 1), tl, ll, np.asarray(s, np.int32))
    x = _leaf(rng, N, T, S, A)
    loss = PrunedStreamingRNNTLoss(blank=A - 1, rnnt_type="regular", delay_penalty=0.3, reduction="none")
    return [x], lambda: loss(x, lab, ttl, tll, rg)


def _mi(N, T, U, rng):
    from warprnnt_pytorch.mi import mutual_information_recursion
    px, py = _leaf(rng, N, U - 1, T + 1), _leaf(rng, N, U, T)
    return [px, py], lambda: mutual_information_recursion(px, py)


def _joiner(layout):
    def build(N, T, U, rng):
        from tests import joiner_forms
        from warprnnt_pytorch import joiner
        tl, ll = _lens(N, T, U)
        ttl, tll = dev(tl, ll)
        f, g = _leaf(rng, N, T, H), _leaf(rng, N, U, H)
        if layout == "padded":
            return [f, g], lambda: joiner.joiner_padded(f, g, ttl, tll, "tanh")
        if layout == "packed":
            return [f, g], lambda: joiner.joiner_packed(f, g, ttl, tll, "tanh")
        rg, = dev(joiner_forms.ranges(dict(N=N, T=T, U=U, S=S), rng))
        return [f, g], lambda: joiner.joiner_pruned(f, g, rg, S, ttl, "tanh")
    return build


WRAPPERS = {"RNNTLoss": _joint(_rnnt), "RNNTLossAdd": _add, "RNNTLossPacked": _packed, "pruned": _pruned, "TDT": _joint(_tdt),
            "HAT": _joint(_hat), "mblank": _joint(_mblank), "mono": _joint(_mono), "AR": _joint(_ar), "KD": _joint(_kd),
            "delay": _joint(_delay), "MI": _mi, "pstream": _pstream, "joiner_padded": _joiner("padded"),
            "joiner_packed": _joiner("packed"), "joiner_pruned": _joiner("pruned")}


def _built(wrapper, shape=0):
    N, T, U = SHAPES[shape]
    rng = np.random.default_rng(100 + shape)
    leaves, forward = WRAPPERS[wrapper](N, T, U, rng)
    out = forward()
    gen = torch.Generator().manual_seed(7 + shape)
    w1, w2 = (torch.randn(out.shape, generator=gen).to(DEV) for _ in range(2))
    return leaves, forward, w1, w2


def _same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert W.same_bits(a, b), "%s: the gradient of input %d differs" % (what, i)
        assert torch.isfinite(a).all() and a.count_nonzero(), what


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_autograd_retain_graph(wrapper):
    """grad with w1, w2, w1 on one retained graph: the first and third equal, the second a fresh graph's."""
    leaves, forward, w1, w2 = _built(wrapper)
    out = forward()
    g1 = torch.autograd.grad(out, leaves, w1, retain_graph=True)
    g2 = torch.autograd.grad(out, leaves, w2, retain_graph=True)
    g3 = torch.autograd.grad(out, leaves, w1)
    _same(g3, g1, "w1 again")
    _same(g2, torch.autograd.grad(forward(), leaves, w2), "w2 against a fresh graph")
    assert not W.same_bits(g1[0], g2[0])


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_autograd_two_backward_calls_accumulate(wrapper):
    leaves, forward, w1, w2 = _built(wrapper)
    want = [a + b for a, b in zip(torch.autograd.grad(forward(), leaves, w1), torch.autograd.grad(forward(), leaves, w2))]
    out = forward()
    out.backward(w1, retain_graph=True)
    out.backward(w2)
    _same([x.grad for x in leaves], want, "two backward calls")


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_autograd_two_graphs_in_reverse_order(wrapper):
    """Two graphs of different shapes built in turn and differentiated in the reverse order: the bits of each alone."""
    a, b = _built(wrapper, 0), _built(wrapper, 1)
    alone = [torch.autograd.grad(forward(), leaves, w1) for leaves, forward, w1, _ in (a, b)]
    out_a, out_b = a[1](), b[1]()
    got_b = torch.autograd.grad(out_b, b[0], b[2])
    got_a = torch.autograd.grad(out_a, a[0], a[2])
    _same(got_a, alone[0], "the first graph, differentiated last")
    _same(got_b, alone[1], "the second graph, differentiated first")
