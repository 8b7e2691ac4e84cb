"""-m gpu: libwarprnnt_joiner.so and warprnnt_pytorch.joiner against the fp64 definition of tests/joiner_ref.py.

Forward.  identity and relu are one rounding of the exact sum: bit-exact against torch's own act(f + g) on the GPU in the same
dtype.  tanh in 16-bit storage: within one quantum of the stored type of the fp64 reference.  tanh in fp32 / fp64: the kernel may
exceed the error torch's own tanh(f + g) has on the same inputs by one ulp -- TANH_ULPS below, measured.

Backward.  Every element of df and dg against the fp64 reference, held to the standard bound of a sum of n terms in any order,
|err| <= (n - 1) u sum|e| with u = 2^-24 (2^-53 for fp64), plus one rounding to the storage type; n and sum|e| come from the
reference, and for tanh e is formed from the stored out that the GPU produced, so the bound is about the reduction.

Coverage.  out, df and dg start as NaN and must be written everywhere, the padding and the label rows without a window as exact
zeros; dout and out hold NaN in every row that is not real, and df and dg must still be finite; two calls give the same bits.
Every kernel form of tests/joiner_forms.py is run and seen to launch."""
import zlib

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import joiner_forms as F
from tests import joiner_ref as R
from tests.gpu_support import CODE, DEV, TORCH, assert_every_row_reached, assert_stages, options, place, profiled, stages_seen

pytestmark = pytest.mark.gpu

# tanh(f + g), fp32 and fp64: the largest error, in ulps of the fp64 reference's value rounded to the type, that torch's own
# tanh(f + g) has on the inputs of test_tanh_against_torchs_own_error (measured on an MI355X: EXPERIMENTS.md section 22),
# plus the one ulp the kernel may exceed it by.
TORCH_TANH_ULPS = {"f32": 1.5921, "f64": 1.0}
TANH_ULPS = {d: None if v is None else v + 1.0 for d, v in TORCH_TANH_ULPS.items()}
U_SUM = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "bf16": 2.0 ** -24, "f16": 2.0 ** -24}         # the accumulator's unit roundoff
U_STORE = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}        # one rounding to the storage type
MANTISSA = {"f32": 23, "f64": 52, "bf16": 7, "f16": 10}
MIN_EXP = {"f32": -126, "f64": -1022, "bf16": -126, "f16": -14}
TORCH_ACT = {"identity": lambda x: x, "relu": torch.relu, "tanh": torch.tanh}


def _jn():
    from warprnnt_pytorch import joiner
    return joiner


def _np(t):
    return t.detach().double().cpu().numpy()


def quantum(ref, dtype):
    """The spacing of `dtype` at |ref| (the subnormal spacing below the smallest normal number)."""
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** MIN_EXP[dtype])))
    return 2.0 ** (e - MANTISSA[dtype])


def store_rounding(ref, dtype):
    """The error one rounding of `ref` to `dtype` can have: half a quantum."""
    return np.maximum(U_STORE[dtype] * np.abs(ref), 0.5 * quantum(np.zeros_like(ref), dtype))


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _fg(name, dtype, N, T, U, H, rng=None):
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    f = torch.tensor(rng.standard_normal((N, T, H)), dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    g = torch.tensor(rng.standard_normal((N, U, H)), dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    return rng, f, g


def _nan_like(shape, dtype, off=0):
    return place(torch.full(shape, float("nan"), dtype=TORCH[dtype], device=DEV), off, TORCH[dtype])


class Problem:
    """One shape of one layout on the device: the index tensors, the C-ABI's argument tail, the reference's arguments."""

    def __init__(self, dtype, layout, act, N, T, U, H, S=0, tl=None, ll=None, ranges=None, off=0, ws=None):
        self.dtype, self.layout, self.act, self.off = dtype, layout, act, off
        self.N, self.T, self.U, self.H, self.S = N, T, U, H, S
        self.tl, self.ll, self.ranges = tl, (None if layout == 2 else ll), ranges
        self.ref_args = (self.tl, self.ll, ranges, S)
        self.shape = R.out_shape(layout, N, T, U, H, self.tl, self.ll, S)
        self.d_tl, self.d_ll = _dev(self.tl, torch.int32), _dev(self.ll, torch.int32)
        self.d_ranges = _dev(ranges, torch.int32) if layout == 2 else None
        self.d_offs = _dev(R.offsets(self.tl, self.ll), torch.int64) if layout == 1 else None
        jn = _jn()
        self.ws_bytes = jn.workspace_bytes(T, U, S, H, N, layout, CODE[dtype])
        self.ws = ws if ws is not None else torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)     # (ws: the caller's)
        ptr = lambda t: None if t is None else t.data_ptr()                 # noqa: E731
        self.tail = (layout, R.ACTS.index(act), ptr(self.d_ranges), S, ptr(self.d_offs), ptr(self.d_ll), ptr(self.d_tl), T, U, H, N,
                     self.ws.data_ptr(), options(T, U), CODE[dtype])
        self.mask = R.real_mask(layout, self.shape, N, T, U, *self.ref_args)

    def flags(self):
        at = -self.ws.data_ptr() % 256
        return self.ws[at:at + 4 * self.N].view(torch.int32).cpu().numpy()

    def fwd(self, f, g):
        out = _nan_like(self.shape, self.dtype, self.off)
        st = _jn().lib().compute_rnnt_joiner_fwd(f.data_ptr(), g.data_ptr(), out.data_ptr(), *self.tail)
        torch.cuda.synchronize()
        assert st == 0
        return out

    def bwd(self, out, dout):
        df = _nan_like((self.N, self.T, self.H), self.dtype, self.off)
        dg = _nan_like((self.N, self.U, self.H), self.dtype, self.off)
        st = _jn().lib().compute_rnnt_joiner_bwd(None if self.act == "identity" else out.data_ptr(), dout.data_ptr(), df.data_ptr(),
                                                 dg.data_ptr(), *self.tail)
        torch.cuda.synchronize()
        assert st == 0
        return df, dg

    def rows(self):
        return R.rows(self.layout, self.N, self.T, self.U, *self.ref_args)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_forward(p, f, g, out, what=""):
    """Coverage and accuracy of `out`; -> the kernel's largest tanh error in ulps (fp32 / fp64), else None."""
    got = _np(out)
    assert np.isfinite(got).all(), (what, "an element of out was not written")
    assert not got[~p.mask].any(), (what, "a row that is not real is not exact zeros")
    rows = p.rows()
    if not rows:
        return None
    bs, ts, us = (torch.tensor([r[i] for r in rows], device=DEV) for i in range(3))
    at = [r[3] for r in rows]
    index = torch.tensor(at, device=DEV) if p.layout == 1 else tuple(torch.tensor(c, device=DEV) for c in zip(*at))
    mine = out[index]                                                              # (rows, H)
    if p.act != "tanh":
        want = TORCH_ACT[p.act](f[:, :, None] + g[:, None])[bs, ts, us]            # torch's own, same dtype, on the GPU
        assert torch.equal(_bits(mine), _bits(want)), (what, "not bit-exact against torch")
        return None
    ref = np.tanh(_np(f)[_np(bs).astype(int), _np(ts).astype(int)] + _np(g)[_np(bs).astype(int), _np(us).astype(int)])
    err = np.abs(_np(mine) - ref) / quantum(ref, p.dtype)
    if p.dtype in ("bf16", "f16"):
        assert err.max() <= 1.0, (what, "tanh: quanta of the stored type", err.max())
        return None
    assert err.max() <= TANH_ULPS[p.dtype], (what, "tanh: ulps", err.max(), TANH_ULPS[p.dtype])
    return err.max()


def poisoned(p, out, dout):
    """Copies of out and dout with NaN in every row that is not real."""
    bad = torch.tensor(~p.mask, device=DEV)
    o, d = out.clone(), dout.clone()
    o[bad] = float("nan")
    d[bad] = float("nan")
    return place(o, p.off, o.dtype), place(d, p.off, d.dtype)


def check_backward(p, out, dout, df, dg, what=""):
    """df and dg against the reference formed from the stored out and dout, element by element."""
    o64, d64 = _np(out), _np(dout)
    rdf, rdg, af, ag, nf, ng = R.backward(o64, d64, p.layout, p.act, p.N, p.T, p.U, *p.ref_args)
    for name, got, ref, a, n in (("df", _np(df), rdf, af, nf), ("dg", _np(dg), rdg, ag, ng)):
        assert np.isfinite(got).all(), (what, name, "not written everywhere, or a row that is not real was read")
        assert not got[n == 0].any(), (what, name, "a row without a term is not exact zeros")
        bound = np.maximum(n - 1, 0)[..., None] * U_SUM[p.dtype] * a + store_rounding(ref, p.dtype) * (n > 0)[..., None]
        err = np.abs(got - ref)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        assert (err <= bound).all(), (what, name, worst, err[worst], bound[worst], int(n[worst[:2]]))


def _dout(p, rng):
    return torch.tensor(rng.standard_normal(p.shape), dtype=torch.float32).to(TORCH[p.dtype]).to(DEV)


def run_and_check(p, f, g, rng, what=""):
    """Forward twice and backward twice with every check; -> the kernel's tanh error in ulps (fp32 / fp64) or None."""
    fo, go = place(f, p.off, f.dtype), place(g, p.off, g.dtype)
    out = p.fwd(fo, go)
    worst = check_forward(p, f, g, out, what)
    assert torch.equal(_bits(out), _bits(p.fwd(fo, go))), (what, "two forward calls differ")
    o_nan, d_nan = poisoned(p, out, _dout(p, rng))
    df, dg = p.bwd(o_nan, d_nan)
    check_backward(p, o_nan, d_nan, df, dg, what)
    df2, dg2 = p.bwd(o_nan, d_nan)
    assert torch.equal(_bits(df), _bits(df2)) and torch.equal(_bits(dg), _bits(dg2)), (what, "two backward calls differ")
    return worst


# ----------------------------------------------------------------------------- the base grid
BASE_TL, BASE_LL = np.array([5, 1, 3], np.int32), np.array([3, 0, 2], np.int32)


@pytest.mark.parametrize("layout,lens", [(0, True), (0, False), (1, True), (2, True), (2, False)])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_base_grid(dtype, act, layout, lens):
    """N = 3, T = 5, U = 4, T_b = (5, 1, 3), L_b = (3, 0, 2): rows off and on the packet boundary (H = 1, 7, 8), a row wider
    than one wave's packets (130), a sample with one frame, a sample with no label; padded and pruned also with lengths NULL."""
    N, T, U, S = 3, 5, 4, 2
    for H in (1, 7, 8, 130):
        what = "%s %s layout %d lens %s H %d" % (dtype, act, layout, lens, H)
        rng, f, g = _fg(what, dtype, N, T, U, H)
        ranges = F.ranges(dict(N=N, T=T, U=U, S=S), rng) if layout == 2 else None
        p = Problem(dtype, layout, act, N, T, U, H, S if layout == 2 else 0, BASE_TL if lens else None, BASE_LL if lens else None,
                    ranges)
        run_and_check(p, f, g, rng, what)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_tanh_against_torchs_own_error(dtype, capsys):
    """torch's own tanh(f + g) on the GPU and the kernel's, both against the fp64 reference on the same inputs, in ulps of the
    type: the kernel may exceed torch's measured error (TORCH_TANH_ULPS) by one ulp.  Both figures are printed."""
    N, T, U, H = 3, 5, 4, 2048
    rng, f, g = _fg("tanh " + dtype, dtype, N, T, U, H)
    ref = np.tanh(_np(f)[:, :, None] + _np(g)[:, None])
    theirs = (np.abs(_np(torch.tanh(f[:, :, None] + g[:, None])) - ref) / quantum(ref, dtype)).max()
    out = Problem(dtype, 0, "tanh", N, T, U, H).fwd(f, g)
    mine = (np.abs(_np(out) - ref) / quantum(ref, dtype)).max()
    with capsys.disabled():
        print("\ntanh %s: torch %.4f ulps, the kernel %.4f ulps" % (dtype, theirs, mine))
    assert TORCH_TANH_ULPS[dtype] is not None and theirs <= TORCH_TANH_ULPS[dtype], (theirs, "the recorded measurement is stale")
    assert mine <= TANH_ULPS[dtype], (mine, TANH_ULPS[dtype])


# ----------------------------------------------------------------------------- every form of tests/joiner_forms.py
def _table_problem(name, case):
    rng, f, g = _fg(name, case["dtype"], case["N"], case["T"], case["U"], case["H"])
    tl, ll = (None, None) if case.get("full") else F.lengths(case, rng)
    ranges = F.ranges(case, rng) if case["layout"] == 2 else None
    p = Problem(case["dtype"], case["layout"], case["act"], case["N"], case["T"], case["U"], case["H"], case["S"], tl, ll, ranges,
                case.get("off", 0))
    return p, f, g, rng


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_joiner_form(name):
    case = F.CASES[name]
    p, f, g, rng = _table_problem(name, case)
    fo, go = place(f, p.off, f.dtype), place(g, p.off, g.dtype)
    dout = _dout(p, rng)

    def both():
        out = p.fwd(fo, go)
        o_nan, d_nan = poisoned(p, out, dout)
        return out, o_nan, d_nan, p.bwd(o_nan, d_nan)
    (out, o_nan, d_nan, (df, dg)), names = profiled(both)
    if not any(F.stage_of(n) for n in names):          # (a profiler session now and then records no device event of the calls
        print(name, "no kernel of the library recorded:", names)      # at all: one more session, judged as the first would have been)
        (out, o_nan, d_nan, (df, dg)), names = profiled(both)
    assert_stages(name, stages_seen(names, F.stage_of, F.STAGES), F.predict(case))
    check_forward(p, f, g, out, name)
    check_backward(p, o_nan, d_nan, df, dg, name)


def test_every_joiner_row_reached_on_this_device():
    assert_every_row_reached(F, G.cus())


# ----------------------------------------------------------------------------- the pruned layout
@pytest.mark.parametrize("which", ["constant", "jumps", "clamp", "s1", "sU"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pruned_windows(dtype, which):
    N, T, U, H = 2, 6, 9, 8
    S = {"s1": 1, "sU": U}.get(which, 3)
    ranges = {"constant": np.full((N, T), 2), "jumps": np.array([[0, 0, 4, 4, 8, 8], [0, 5, 5, 5, 5, 6]]),
              "clamp": np.array([[5, 6, 7, 7, 8, 8], [8, 8, 8, 8, 8, 8]]), "s1": np.array([[0, 1, 3, 3, 8, 8], [0, 0, 0, 0, 0, 0]]),
              "sU": np.array([[0, 0, 0, 0, 0, 0], [0, 2, 4, 6, 8, 8]])}[which].astype(np.int32)
    rng, f, g = _fg("windows " + which + dtype, dtype, N, T, U, H)
    for tl in (None, np.array([T, 4], np.int32)):
        p = Problem(dtype, 2, "tanh", N, T, U, H, S, tl, None, ranges)
        run_and_check(p, f, g, rng, which)
    _, _, _, _, _, ng = R.backward(np.zeros(p.shape), np.zeros(p.shape), 2, "identity", N, T, U, None, None, ranges, S)
    if which == "jumps":
        assert (ng[0] == 0).any()                                      # label rows no window covers
    if which == "clamp":
        assert ng[1, U - 1] == T * S                                   # every slot of sample 1 lands on the last row
    # the forward is bit-for-bit act(am_p + lm_p) of prune_inputs for identity and relu (lengths NULL)
    from warprnnt_pytorch.pruned import prune_inputs
    for act in ("identity", "relu"):
        am_p, lm_p = prune_inputs(f, g, _dev(ranges), S)
        out = _jn().joiner_pruned(f, g, _dev(ranges), S, None, act)
        assert torch.equal(_bits(out), _bits(TORCH_ACT[act](am_p + lm_p))), (which, act)


def test_bad_starts_zero_their_sample_and_raise_its_flag():
    jn = _jn()
    N, T, U, H, S = 3, 5, 4, 8, 2
    rng, f, g = _fg("bad starts", "f32", N, T, U, H)
    ranges = F.ranges(dict(N=N, T=T, U=U, S=S), rng)
    good = ranges.copy()
    ranges[1, 0], ranges[1, 3] = -1, U                   # both in one sample
    ranges[2, 4] = 17                                    # frame 4 of sample 2 is not read (T_2 = 3)
    tl = np.array([5, 5, 3], np.int32)
    f.requires_grad_(True)
    g.requires_grad_(True)
    out, flags = jn.joiner_pruned(f, g, _dev(ranges), S, _dev(tl), "tanh", validate=False, return_flags=True)
    assert flags.cpu().tolist() == [0, 1, 0]
    dout = torch.randn_like(out)
    out.backward(dout)
    ref, flags0 = jn.joiner_pruned(f.detach(), g.detach(), _dev(good), S, _dev(tl), "tanh", validate=False, return_flags=True)
    assert flags0.cpu().tolist() == [0, 0, 0]
    assert not out[1].any() and torch.equal(_bits(out[0]), _bits(ref[0])) and torch.equal(_bits(out[2]), _bits(ref[2]))
    assert not f.grad[1].any() and not g.grad[1].any() and f.grad[0].any() and g.grad[2].any()
    assert torch.isfinite(f.grad).all() and torch.isfinite(g.grad).all()
    p = Problem("f32", 2, "tanh", N, T, U, H, S, tl, None, ranges)
    check_backward(p, out.detach(), dout, f.grad, g.grad, "bad starts")
    with pytest.raises(ValueError, match="ranges of sample 1 start outside"):
        jn.joiner_pruned(f, g, _dev(ranges), S, _dev(tl), "tanh")


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_gradcheck_fp64(layout, act):
    jn = _jn()
    N, T, U, H, S = 2, 3, 3, 4, 2
    rng, f, g = _fg("gradcheck %d %s" % (layout, act), "f64", N, T, U, H)
    tl, ll = _dev(np.array([3, 2], np.int32)), _dev(np.array([2, 1], np.int32))
    ranges = _dev(np.array([[0, 1, 2], [0, 0, 1]], np.int32))
    fn = {0: lambda a, b: jn.joiner_padded(a, b, tl, ll, act), 1: lambda a, b: jn.joiner_packed(a, b, tl, ll, act),
          2: lambda a, b: jn.joiner_pruned(a, b, ranges, S, tl, act)}[layout]
    assert torch.autograd.gradcheck(fn, (f.requires_grad_(True), g.requires_grad_(True)), eps=1e-6, atol=1e-7, rtol=1e-6,
                                    nondet_tol=0.0)


def _grads(loss, *leaves):
    for t in leaves:
        t.grad = None
    loss.backward()
    return [t.grad.clone() for t in leaves]


def _close(a, b, tol=1e-10):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_packed_route_equals_padded_route(act):
    """joiner_packed -> Linear -> RNNTLossPacked equals joiner_padded -> Linear -> RNNTLoss, fp64, to 1e-10."""
    from warprnnt_pytorch import RNNTLoss
    from warprnnt_pytorch.packed import RNNTLossPacked
    jn = _jn()
    N, T, U, H, A = 3, 6, 4, 8, 5
    rng, f, g = _fg("routes packed " + act, "f64", N, T, U, H)
    f.requires_grad_(True), g.requires_grad_(True)
    lin = torch.nn.Linear(H, A).double().to(DEV)
    tl, ll = _dev(np.array([6, 2, 4], np.int32)), _dev(np.array([3, 0, 2], np.int32))
    labels = _dev(rng.integers(1, A, size=(N, U - 1)).astype(np.int32))
    leaves = (f, g, lin.weight, lin.bias)
    a = RNNTLossPacked(reduction="sum")(lin(jn.joiner_packed(f, g, tl, ll, act)), labels, tl, ll)
    ga = _grads(a, *leaves)
    b = RNNTLoss(reduction="sum")(lin(jn.joiner_padded(f, g, tl, ll, act)), labels, tl, ll)
    gb = _grads(b, *leaves)
    assert _close(a.detach(), b.detach()) and all(_close(x, y) for x, y in zip(ga, gb))
    assert torch.isfinite(a).all() and all(x.abs().max() > 0 for x in gb)


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_pruned_route_equals_the_torch_route(act):
    """joiner_pruned -> Linear -> RNNTLossPruned equals prune_inputs -> add -> act -> Linear -> RNNTLossPruned, fp64, to 1e-10."""
    from tests import pstream_forms
    from warprnnt_pytorch.pruned import RNNTLossPruned, prune_inputs
    jn = _jn()
    case = dict(N=4, T=7, U=5, S=3, type=0)
    N, T, U, S, H, A = 4, 7, 5, 3, 8, 6
    rng, f, g = _fg("routes pruned " + act, "f64", N, T, U, H)
    f.requires_grad_(True), g.requires_grad_(True)
    tl_np, ll_np = pstream_forms.lengths(case, rng)
    ranges = _dev(pstream_forms.ranges(case, tl_np, ll_np, rng))
    tl, ll = _dev(tl_np), _dev(ll_np)
    lin = torch.nn.Linear(H, A).double().to(DEV)
    labels = _dev(rng.integers(1, A, size=(N, U - 1)).astype(np.int32))
    leaves = (f, g, lin.weight, lin.bias)
    loss = RNNTLossPruned(reduction="sum")
    a = loss(lin(jn.joiner_pruned(f, g, ranges, S, tl, act)), labels, tl, ll, ranges)
    ga = _grads(a, *leaves)
    am_p, lm_p = prune_inputs(f, g, ranges, S)
    b = loss(lin(TORCH_ACT[act](am_p + lm_p)), labels, tl, ll, ranges)
    gb = _grads(b, *leaves)
    assert _close(a.detach(), b.detach()) and all(_close(x, y) for x, y in zip(ga, gb))
    assert torch.isfinite(a).all() and all(x.abs().max() > 0 for x in gb)


def test_transducer_joint_module():
    jn = _jn()
    N, T, U, H = 3, 5, 4, 8
    _, f, g = _fg("module", "bf16", N, T, U, H)
    f_len, g_len = _dev(BASE_TL.astype(np.int64)), _dev(BASE_LL.astype(np.int64) + 1)
    tl, ll = _dev(BASE_TL), _dev(BASE_LL)
    assert torch.equal(_bits(jn.TransducerJoint()(f, g, f_len, g_len)), _bits(jn.joiner_padded(f, g, tl, ll, "relu")))
    packed = jn.TransducerJoint("tanh", pack_output=True)(f, g, f_len, g_len)
    assert packed.shape == (int((BASE_TL * (BASE_LL + 1)).sum()), H)
    assert torch.equal(_bits(packed), _bits(jn.joiner_packed(f, g, tl, ll, "tanh")))


def test_python_refusals_on_the_device():
    jn = _jn()
    _, f, g = _fg("refusals", "f32", 3, 5, 4, 8)
    tl, ll = _dev(BASE_TL), _dev(BASE_LL)
    for bad_f, bad_g, text in ((f.double(), g, "one dtype"), (f.transpose(0, 1).contiguous().transpose(0, 1), g, "contiguous"),
                               (f, g[:, :, :4].contiguous(), r"f must be \(N, T, H\)"), (f.cpu(), g, "GPU only")):
        with pytest.raises(ValueError, match=text):
            jn.joiner_padded(bad_f, bad_g, tl, ll)
    with pytest.raises(ValueError, match="act_lens exceed f"):
        jn.joiner_padded(f, g, _dev(np.array([6, 1, 3], np.int32)), ll)
    with pytest.raises(ValueError, match="label_lens exceed g"):
        jn.joiner_packed(f, g, tl, _dev(np.array([4, 0, 2], np.int32)))
    with pytest.raises(ValueError, match="act_lens must be a torch.int32 tensor"):
        jn.joiner_padded(f, g, tl.long(), ll)
    with pytest.raises(ValueError, match="on the device of f"):
        jn.joiner_padded(f, g, tl.cpu(), ll)
    with pytest.raises(ValueError, match=r"S must be in \[1, maxU\]"):
        jn.joiner_pruned(f, g, _dev(np.zeros((3, 5), np.int32)), 5)
    with pytest.raises(ValueError, match="rows = 3"):
        jn.joiner_packed(f, g, tl, ll, rows=3)


# ----------------------------------------------------------------------------- graph capture
def test_hip_graph_capture_and_replay():
    """joiner_packed(rows=R, validate=False) forward and backward captured and replayed on changed inputs gives the eager bits."""
    jn = _jn()
    N, T, U, H = 3, 5, 4, 16
    rng, f, g = _fg("graph", "f32", N, T, U, H)
    tl, ll = _dev(BASE_TL), _dev(BASE_LL)
    offsets = _dev(R.offsets(BASE_TL, BASE_LL), torch.int64)
    rows = int(R.offsets(BASE_TL, BASE_LL)[-1])
    dout = torch.randn(rows, H, device=DEV)
    f.requires_grad_(True), g.requires_grad_(True)

    def step():
        out = jn.joiner_packed(f, g, tl, ll, "tanh", offsets=offsets, rows=rows, validate=False)
        df, dg = torch.autograd.grad(out, (f, g), dout)
        return out, df, dg
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in range(2):
        with torch.no_grad():
            f.copy_(torch.randn(N, T, H, generator=torch.Generator().manual_seed(seed)))
            g.copy_(torch.randn(N, U, H, generator=torch.Generator().manual_seed(10 + seed)))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        eager = step()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(replayed, eager))
        assert all(torch.isfinite(t).all() and t.abs().max() > 0 for t in replayed)
