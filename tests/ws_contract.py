"""The workspace contract of every library, through one harness (not collected, not a conftest).

Every entry of the project takes a caller-owned workspace of get_workspace_size*() bytes.  The contract: a call writes nothing
outside those bytes, whatever the buffer held on entry changes no bit of any output, and a workspace that a forward call left
serves any number of backward calls.  REGISTRY has one Library per sizing function the headers declare; a Library turns a case of
its forms tables (tests/*_forms.py) into Problems -- the healthy batch the table describes, the same dims with every sample on
a failure route the header documents, and a healthy batch of other dims (N + 1, T + 3, U + 2) -- and a Problem runs one C-ABI
form on a workspace it is handed: run(ws, form, scale) -> {name: output}.  Forms: `one` (one call with gradients), `score`
(no gradients), `two` (_fwd(prepare_backward = 1) then _bwd with a per-sample scale) and its halves `fwd` and `bwd`.  The side
libraries go through their test module's `call` helper and gpu_support.call_forms, with the workspace passed as ws=.

check_case() is the whole contract for one (library, case); tests/test_gpu_ws_contract.py runs it for every case.  Every
comparison is of bits against the bits the same form gives on a zero-filled workspace (which the module's own test_*_form holds
to the fp64 reference): no tolerance anywhere -- but for the additive joint, whose float atomics leave the last bits of df and dg
to the order the blocks arrive in (class _Add): a run of it whose bits differ is held to its module's own oracle check.  The main
library's host-cost entries (compute_rnnt_loss and its per-dtype twins) are compute_rnnt_loss_async's driver, run_gpu, with the
costs copied to the host: their cases run through the async entry.
The judges (same_bits, differing, Workspace.guards_intact) and the leave-out rule (uncovered) need no GPU:
tests/test_ws_contract_cpu.py plants faults into them."""
import importlib
import zlib

import numpy as np
import torch

GUARD = 4096            # bytes in front of and behind the workspace
PATTERN = 0xA5          # what the guards hold
SHIFT = 8               # the second placement: this far past a 256-byte boundary (every sizing function has the align_up slack)
GROW = dict(N=1, T=3, U=2)
LIMIT = 8 << 20         # elements of a case's largest tensor from which it may be left out (if its kernels stay covered)
MAX_U = 1024            # the main library and the additive joint: one lane per label position (make_plan, csrc/rnnt_host.h)
DEV = "cuda:0"


# ----------------------------------------------------------------------------- the judges
def _tensor(v):
    return torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach().cpu().contiguous()


def bits(v):
    """The bytes of an array or tensor, flat."""
    return _tensor(v).reshape(-1).view(torch.uint8)


def same_bits(a, b):
    ta, tb = _tensor(a), _tensor(b)
    return ta.shape == tb.shape and ta.dtype == tb.dtype and torch.equal(bits(ta), bits(tb))


def differing(got, want):
    """The names of the outputs whose bits differ between two runs (an output only one run has differs)."""
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or not same_bits(got[k], want[k]))


def assert_same(got, want, what):
    bad = differing(got, want)
    assert not bad, "%s: %s differ%s from the reference run's" % (what, ", ".join(bad), "s" if len(bad) == 1 else "")


class Workspace:
    """`nbytes` of workspace, `shift` bytes past a 256-byte boundary, between two guards of GUARD bytes of PATTERN."""

    def __init__(self, nbytes, shift=0, fill=0, device=DEV):
        self.nbytes, self.lo, self.hi = nbytes, GUARD + shift, GUARD + shift + nbytes
        self.buf = torch.full((self.hi + GUARD,), PATTERN, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 256 == 0 or self.buf.device.type == "cpu"
        self.ws = self.buf[self.lo:self.hi]
        self.ws.fill_(fill)

    def data_ptr(self):
        return self.ws.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.lo] == PATTERN).all()) and bool((self.buf[self.hi:] == PATTERN).all())

    def assert_guards(self, what):
        lo, hi = self.buf[:self.lo].cpu(), self.buf[self.hi:].cpu()
        for name, g, at in (("in front of", lo, -self.lo), ("behind", hi, self.nbytes)):
            bad = (g != PATTERN).nonzero().reshape(-1)
            assert not bad.numel(), ("%s: %d bytes written %s the workspace of %d bytes, the first at byte %d"
                                     % (what, bad.numel(), name, self.nbytes, at + int(bad[0])))


# ----------------------------------------------------------------------------- problems
class Problem:
    """One batch of one library on the device.  nbytes: the sizing function's answer for its dims; forms: the call forms the
    library has for it, of one | score | two; halves: `two` also runs as fwd and bwd on their own; N: samples (the scales)."""
    forms = ("one", "score", "two")
    halves = True
    failed = None                   # the failing batch: failed(outputs) asserts what the header documents
    judge = None                    # a library that sums with float atomics: judge(outputs, form, scale), its module's own check

    @property
    def primary(self):
        """The first form with gradients (a library without any: its one form)."""
        return next((f for f in self.forms if f != "score"), self.forms[0])

    def run(self, ws, form, scale=None):
        raise NotImplementedError


def scales(N, which):
    """Two per-sample scales, none of them 1."""
    return (0.625 + 0.25 * np.arange(N)) if which == 1 else (1.875 - 0.375 * (np.arange(N) % 4))


class Called(Problem):
    """A side library through its test module's `call` helper: call(form=, scale=, ws=) -> (status, *outputs)."""

    def __init__(self, nbytes, N, call, names=("costs", "grads"), forms=Problem.forms, halves=True):
        self.nbytes, self.N, self._call, self.names, self.forms, self.halves = nbytes, N, call, names, forms, halves

    def run(self, ws, form, scale=None):
        st, *out = self._call(form, scale, ws)
        assert st == 0, (form, st)
        return {n: v for n, v in zip(self.names, out) if v is not None and (form != "bwd" or "grad" in n)}     # (bwd: gradients)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _grown(case, keys=("N", "T", "U"), max_u=None, **kw):
    """The case at other dims: N + 1, T + 3, U + 2 -- U - 2 where the library takes no more than max_u label positions."""
    grow = dict(GROW, U=-GROW["U"]) if max_u is not None and case["U"] + GROW["U"] > max_u else GROW
    return dict(case, name=case["name"] + "_grown", **{k: case[k] + grow[{"S": "U"}.get(k, k)] for k in keys}, **kw)


def spoil_rows(*tensors):
    """NaN over the first row of every sample that the healthy batch reads (its values are finite: every row that is never
    read holds NaN already), in the first tensor that has one: a non-finite in-lattice row, the failure route every header
    documents (cost NaN, NaN gradients on the sample's in-lattice rows).  -> the spoiled copies, the samples spoiled."""
    out = [t.clone() for t in tensors]
    hit = []
    for b in range(out[0].shape[0]):
        for t in out:
            live = torch.isfinite(t[b].float()).all(-1).reshape(-1).nonzero().reshape(-1)
            if live.numel() and t.shape[-1]:
                t[b].reshape(-1, t.shape[-1])[int(live[0])] = float("nan")
                hit.append(b)
                break
    assert hit, "no sample has a row that is read"
    return out, hit


def _non_finite(hit, cost="costs", grads=("grads",)):
    """No spoiled sample has a finite cost, one at least has NaN (a sample without a path keeps its +-inf), and every sample
    with a NaN cost has NaN in a gradient."""
    def failed(out):
        c = np.asarray(out[cost], np.float64)
        assert not np.isfinite(c[hit]).any() and np.isnan(c[hit]).any(), (cost, out[cost])
        have = [g for g in grads if g in out and out[g].size]
        for b in hit:
            assert not have or np.isinf(c[b]) or any(np.isnan(out[g][b]).any() for g in have), (b, "NaN cost, no NaN gradient")
    return failed


def _placed(x, off):
    from tests.gpu_support import place
    return place(x.to(DEV), off, x.dtype)


def _nan_grads(x, off):
    return _placed(torch.full_like(x, float("nan")), off)


def _logits_library(module, build, nbytes, names=("costs", "grads")):
    """problem(case, variant) of a loss on one logits tensor: build(M, case) -> (x, rest, kw, mask) with M.call(x, *rest, **kw,
    form=, scale=, grads=, ws=) and mask the rows the module's checker compares (tests/side_limits.py repeats such a batch);
    the failing batch is the healthy one with a NaN row in every sample."""
    def problem(case, variant, cus):
        M = importlib.import_module("tests.test_gpu_" + module)
        case = _resolve(case, cus)
        if variant == "grown":
            case = _grown(case, lengths=None) if "lengths" in case else _grown(case)
        x, rest, kw, _ = build(M, case)
        off = case.get("off", 0)
        hit = None
        if variant == "failing":
            (x,), hit = spoil_rows(x)
        xd = _placed(x, off)
        kw = {k: (_placed(v, off + case.get("toff", 0)) if torch.is_tensor(v) else v) for k, v in kw.items()}
        rest = [_placed(v, off + case.get("toff", 0)) if torch.is_tensor(v) else v for v in rest]
        p = Called(nbytes(M, case, xd), xd.shape[0],
                   lambda form, scale, ws: M.call(xd, *rest, **kw, form=form, scale=scale, grads=_nan_grads(xd, off), ws=ws), names)
        if hit is not None:
            p.failed = _non_finite(hit)
        return p
    return problem


def _resolve(case, cus):
    """A case whose N is relative to the compute-unit count (tests/kernel_forms.py: case_shape), with its number."""
    if isinstance(case.get("N"), str):
        from tests import kernel_forms as K
        return dict(case, N=K.case_shape(case, cus)[0])
    return case


def _code(x):
    from tests.gpu_support import CODE, NAME
    return CODE[NAME[x.dtype]]


# ----------------------------------------------------------------------------- the side libraries
def _lengths(c):
    """A case's own (T_b, L_b), where it has them (tests/side_limits.py: full-length samples); else the module's ragged ones."""
    ln = c.get("lengths")
    return None if ln is None else (np.asarray(ln[0], np.int32), np.asarray(ln[1], np.int32))


def _pruned(M, c):
    x, labels, tl, ll, ranges, mask = M._problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["S"],
                                                 lengths=_lengths(c))
    return x, (labels, tl, ll, ranges, c["S"], c["U"]), {}, mask


def _hat(M, c):
    x, labels, tl, ll, mask = M._problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["blank"],
                                         lengths=_lengths(c))
    return x, (labels, tl, ll), dict(blank=c["blank"]), mask


def _tdt(M, c):
    x, labels, tl, ll, mask = M._problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["durations"],
                                         lengths=_lengths(c))
    return x, (labels, tl, ll, c["durations"]), {}, mask


def _mblank(M, c):
    x, labels, tl, ll, mask = M._problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["blank"], c["columns"],
                                         lengths=_lengths(c))
    return x, (labels, tl, ll, c["columns"], c["durations"]), dict(blank=c["blank"]), mask


def _kd(M, c):
    z, w, labels, tl, ll, mask = M._problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["blank"],
                                            lengths=_lengths(c))
    return z, (w, labels, tl, ll), dict(blank=c["blank"], mode=c["mode"], tau=1.0), mask


def _ar(M, c):
    x, labels, tl, ll, lo, hi, mask = M._table_problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["blank"])
    return x, (labels, tl, ll, lo, hi), dict(blank=c["blank"]), mask


def _delay(M, c):
    x, labels, tl, ll, mask = M._table_problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], c["blank"])
    return x, (labels, tl, ll), dict(blank=c["blank"]), mask


def _pstream(M, c):
    x, labels, s, tl, ll, mask = M._table_problem(c["name"], c)
    return x, (labels, s, tl, ll, c["U"]), dict(blank=c["blank"], typ=c["type"]), mask


def _mono(M, c):
    from tests import mono_forms as F
    rng = _rng(c["name"])
    x, labels, tl, ll, mask = M._problem(c["name"], c["dtype"], c["N"], c["T"], c["U"], c["A"], F.lengths(c, rng), rng=rng,
                                         blank=c["blank"])
    return x, (labels, tl, ll), dict(blank=c["blank"]), mask


def _pruned_problem(case, variant, cus):
    """The pruned loss and, for the table's `ranges` cases, compute_rnnt_prune_ranges_add on the same workspace.  The failing
    batch: a window start outside [0, L_b] in every sample (the invalid-arguments cost marker, a NaN); for a `ranges` case it
    is the loss on the same N, maxT, maxU."""
    from tests import test_gpu_pruned as M
    from tests.gpu_support import CODE, TORCH, dev, options, ragged_lengths
    case = _resolve(case, cus)
    if variant == "grown":
        case = _grown(case)
    N, T, U, A, S, dtype = case["N"], case["T"], case["U"], case["A"], case["S"], case["dtype"]
    nbytes = M._pl().workspace_bytes(T, U, N, CODE[dtype])
    if case["entry"] == "ranges" and variant != "failing":
        rng = _rng(case["name"])
        tl, ll = ragged_lengths(N, T, U, rng)
        off = case.get("off", {})
        f = _placed(torch.tensor(rng.standard_normal((N, T, A)), dtype=torch.float32).to(TORCH[dtype]), off.get("f", 0))
        g = _placed(torch.tensor(rng.standard_normal((N, U, A)), dtype=torch.float32).to(TORCH[dtype]), off.get("g", 0))
        labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32) if A > 1 else np.zeros((N, U - 1), np.int32)
        lab, ttl, tll = dev(labels, tl, ll)

        def call(form, scale, ws):
            out = torch.full((N, T), -7, dtype=torch.int32, device=DEV)
            st = M._pl().lib().compute_rnnt_prune_ranges_add(f.data_ptr(), g.data_ptr(), lab.data_ptr(), tll.data_ptr(),
                                                             ttl.data_ptr(), A, N, S, out.data_ptr(), ws.data_ptr(),
                                                             options(T, U), CODE[dtype])
            torch.cuda.synchronize()
            return st, out.cpu().numpy()
        return Called(nbytes, N, call, ("ranges",), forms=("one",), halves=False)
    if case["entry"] == "ranges":
        A, case = min(A, 8), dict(case, off=0)
    x, (labels, tl, ll, ranges, _, _), _, _ = _pruned(M, dict(case, N=N, T=T, U=U, A=A))
    if variant == "failing":
        x = torch.nan_to_num(x)
        ranges = ranges.copy()
        ranges[:, 0] = ll + 1
    off = case.get("off", 0)
    xd = _placed(x, off)
    p = Called(nbytes, N, lambda form, scale, ws: M.call(xd, labels, tl, ll, ranges, S, U, form=form, scale=scale,
                                                         grads=_nan_grads(xd, off), ws=ws))
    if variant == "failing":
        def failed(out):
            assert np.isnan(out["costs"]).all(), out["costs"]
        p.failed = failed
    return p


def _mi_problem(case, variant, cus):
    """The failing batch: a NaN on an edge inside every rectangle that has one (NaN score, NaN gradients on its edges)."""
    from tests import test_gpu_mi as M
    from tests.gpu_support import CODE
    if variant == "grown":
        case = _grown(case, keys=("N", "T", "S"))
    px, py, bd, _, _ = M._table_problem(case)
    hit = None
    if variant == "failing":
        (py, px), hit = _spoil_edges(py, px)
    xd, yd = px.to(DEV), py.to(DEV)
    nbytes = M._mi().workspace_bytes(case["S"], case["T"], case["N"], int(case["mod"]), CODE[case["dtype"]])
    p = Called(nbytes, case["N"], lambda form, scale, ws: M.call(xd, yd, bd, form, scale, ws=ws), ("scores", "px_grad", "py_grad"))
    if hit is not None:
        p.failed = _non_finite(hit, "scores", ("px_grad", "py_grad"))
    return p


def _spoil_edges(*tensors):
    """spoil_rows for edge weights: one finite ELEMENT per sample (a -inf weight is routine there, a whole row is not needed)."""
    out = [t.clone() for t in tensors]
    hit = []
    for b in range(out[0].shape[0]):
        for t in out:
            live = torch.isfinite(t[b].float()).reshape(-1).nonzero().reshape(-1)
            if live.numel():
                t[b].reshape(-1)[int(live[0])] = float("nan")
                hit.append(b)
                break
    assert hit, "no sample has an edge that is read"
    return out, hit


def _tdt_align_problem(case, variant, cus):
    """One enqueue: score, frames, durs.  The failing batch: a NaN row inside every lattice (score NaN, frames and durs -1)."""
    from tests import test_gpu_tdt_align as M
    if variant == "grown":
        case = _grown(case)
    N, T, U, A, durs = case["N"], case["T"], case["U"], case["A"], case["durations"]
    x, labels, tl, ll, _ = M._problem(case["name"], case["dtype"], N, T, U, A, durs)
    hit = None
    if variant == "failing":
        (x,), hit = spoil_rows(x)
    xd = _placed(x, case.get("off", 0))
    p = Called(M._mod().workspace_bytes(T, U, N, len(durs), _code(xd)), N,
               lambda form, scale, ws: M.call(xd, labels, tl, ll, durs, ws=ws), ("score", "frames", "durs"), forms=("one",),
               halves=False)
    if hit is not None:
        def failed(out):
            assert np.isnan(out["score"][hit]).all() and (out["frames"][hit] == -1).all() and (out["durs"][hit] == -1).all(), out
        p.failed = failed
    return p


def _joiner_problem(case, variant, cus):
    """fwd then bwd on one workspace: out, df, dg and, in the pruned layout, the flags.  The failing batch: the pruned layout on
    the same dims with a window start outside [0, U - 1] in every sample (every flag 1, every row zeros)."""
    from tests import joiner_forms as F
    from tests import test_gpu_joiner as M
    if variant == "grown":
        case = _grown(case)
    if variant == "failing":
        case = dict(case, layout=2, S=max(case["S"], 1), full=False, off=0)
    name = case["name"]
    rng, f, g = M._fg(name, case["dtype"], case["N"], case["T"], case["U"], case["H"])
    tl, ll = (None, None) if case.get("full") else F.lengths(case, rng)
    ranges = F.ranges(case, rng) if case["layout"] == 2 else None
    if variant == "failing":
        ranges[:, 0] = case["U"]
    off = case.get("off", 0)
    fo, go = M.place(f, off, f.dtype), M.place(g, off, g.dtype)
    seed = int(rng.integers(1 << 30))
    nbytes = M._jn().workspace_bytes(case["T"], case["U"], case["S"], case["H"], case["N"], case["layout"], M.CODE[case["dtype"]])

    def call(form, scale, ws):
        p = M.Problem(case["dtype"], case["layout"], case["act"], case["N"], case["T"], case["U"], case["H"], case["S"], tl, ll,
                      ranges, off, ws=ws)
        out = p.fwd(fo, go)
        o_nan, d_nan = M.poisoned(p, out, M._dout(p, np.random.default_rng(seed)))
        df, dg = p.bwd(o_nan, d_nan)
        at = -ws.data_ptr() % 256
        flags = ws.ws[at:at + 4 * p.N].view(torch.int32).cpu() if case["layout"] == 2 else None
        return 0, out.cpu(), df.cpu(), dg.cpu(), flags
    p = Called(nbytes, case["N"], call, ("out", "df", "dg", "flags"), forms=("one",), halves=False)
    if variant == "failing":
        def failed(out):
            assert (out["flags"] == 1).all() and not out["out"].count_nonzero() and not out["df"].count_nonzero(), out["flags"]
        p.failed = failed
    return p


# ----------------------------------------------------------------------------- the main library
class _Main(Problem):
    """The materialised path (padded: compute_rnnt_loss_async, _fwd + _bwd; packed: compute_rnnt_loss_packed, _packed_fwd +
    _packed_bwd) on a case of tests/kernel_forms.py, as tests/test_gpu_kernel_forms.py builds it.  `one` carries the case's own
    scale (the kernel form depends on it), `two` the harness's.  The failing batch: a NaN logit in row (0, 0) of every sample."""

    def __init__(self, case, variant, cus):
        from tests import kernel_forms as K
        from tests.gpu_support import TORCH
        from tests.test_gpu_kernel_forms import _inputs, _scale
        from warprnnt_pytorch import _lib
        from warprnnt_pytorch.packed import pack_joint, row_offsets
        case = _resolve(case, cus)
        if variant == "grown":
            case = _grown(case, max_u=MAX_U)
        self.case, self.lib = case, _lib.lib()
        N, T, U, A = K.case_shape(case, cus)
        x, labels, tl, ll, blank = _inputs(case, cus, _rng(case["name"]))
        dt = TORCH[case["dtype"]]
        self.code, esz = {torch.float32: (_lib.DT_F32, 4), torch.float64: (_lib.DT_F64, 8), torch.bfloat16: (_lib.DT_BF16, 2),
                          torch.float16: (_lib.DT_F16, 2)}[dt]
        self.cdt = torch.float64 if dt == torch.float64 else torch.float32
        self.N, self.A, self.nbytes = N, A, _lib.workspace_bytes(T, U, N, True, esz)
        self.own_scale = _scale(case, N, dt)
        self.lab, self.tl, self.ll = (torch.tensor(v, device=DEV) for v in (labels, tl, ll))
        self.opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream().cuda_stream,
                                    blank_label=blank, maxT=T, maxU=U, batch_first=True)
        self.packed = case.get("layout") == "packed"
        if variant == "failing":
            x[:, 0, 0, 0] = float("nan")
            self.failed = _non_finite(list(range(N)))
        if self.packed:
            self.x = pack_joint(x.to(DEV), self.tl, self.ll).contiguous()
            self.offs = row_offsets(self.tl, self.ll)
            self.rows = self.x.shape[0]
        else:
            for b in range(N):                                       # NaN in every padded row: must never be read
                x[b, tl[b]:] = float("nan")
                x[b, :, ll[b] + 1:] = float("nan")
            self.x = x.to(DEV)
        self.aux = torch.cuda.Stream() if case.get("aux") else None

    def _grads(self):
        if self.case.get("misalign"):                                # grads at another 16-byte phase than acts
            buf = torch.full((self.x.numel() + 1,), float("nan"), dtype=self.x.dtype, device=DEV)
            return buf[1:].view(self.x.shape)
        return torch.full_like(self.x, float("nan"))

    def run(self, ws, form, scale=None):
        from warprnnt_pytorch import warp_rnnt
        lib, x, opt, code, A, N = self.lib, self.x.data_ptr(), self.opt, self.code, self.A, self.N
        lens = (self.lab.data_ptr(), self.ll.data_ptr(), self.tl.data_ptr())
        costs = torch.full((N,), float("nan"), dtype=self.cdt, device=DEV)
        g = None if form in ("score", "fwd") else self._grads()
        gp = None if g is None else g.data_ptr()
        sc = self.own_scale if form == "one" else scale
        t_sc = None if sc is None else torch.tensor(np.asarray(sc), dtype=self.cdt, device=DEV)
        sp = None if t_sc is None else t_sc.data_ptr()
        if self.aux is not None:
            warp_rnnt.set_aux_stream(self.aux)
        try:
            st = 0
            if self.packed:
                tail = (self.offs.data_ptr(), self.rows, A, N)
                if form in ("one", "score"):
                    st = lib.compute_rnnt_loss_packed(x, gp, *lens, *tail, costs.data_ptr(), sp if form == "one" else None,
                                                      ws.data_ptr(), opt, code, 0.0)
                else:
                    if form != "bwd":
                        st = lib.compute_rnnt_loss_packed_fwd(x, *lens, *tail, costs.data_ptr(), ws.data_ptr(), opt, code, 1, 0.0)
                    if form != "fwd" and st == 0:
                        st = lib.compute_rnnt_loss_packed_bwd(x, gp, sp, *tail, ws.data_ptr(), opt, code)
            elif form in ("one", "score"):
                st = lib.compute_rnnt_loss_async(x, gp, *lens, A, N, costs.data_ptr(), sp if form == "one" else None,
                                                 ws.data_ptr(), opt, code)
            else:
                if form != "bwd":
                    st = lib.compute_rnnt_loss_fwd(x, *lens, A, N, costs.data_ptr(), ws.data_ptr(), opt, code, 1)
                if form != "fwd" and st == 0:
                    st = lib.compute_rnnt_loss_bwd(x, gp, sp, A, N, ws.data_ptr(), opt, code)
            torch.cuda.synchronize()
        finally:
            if self.aux is not None:
                warp_rnnt.set_aux_stream(None)
        assert st == 0, (form, st)
        out = {} if form == "bwd" else {"costs": costs.cpu().numpy()}
        if g is not None:
            out["grads"] = g.double().cpu().numpy()
        if form != "bwd":                                            # the likelihoods the workspace keeps
            llf, llb = np.zeros(N), np.zeros(N)
            assert lib.compute_rnnt_loss_likelihoods(ws.data_ptr(), N, opt, code, llf.ctypes.data, llb.ctypes.data) == 0
            out["ll_forward"] = llf
            if form != "score":
                out["ll_backward"] = llb
        return out


class _Align(Problem):
    """compute_rnnt_align (materialised) or compute_rnnt_align_add on an alignment case of tests/joint_forms.py: score and
    frames.  The failing batch: a NaN in row (0, 0) of every sample (score NaN, frames -1)."""
    forms, halves = ("one",), False

    def __init__(self, case, variant, cus):
        from tests import joint_forms as J
        from tests.gpu_support import TORCH, options, ragged_lengths
        from tests.test_gpu_joint_forms import _nan_padding, _planted
        from warprnnt_pytorch import _lib
        case = _resolve(case, cus)
        if variant == "grown":
            case = _grown(case, max_u=MAX_U)
        N, T, U, A = J.K.case_shape(case, cus)
        dt = TORCH[case["dtype"]]
        rng = _rng(case["name"])
        planted = case.get("data") == "planted"
        if planted:
            acts, labels = _planted(N, T, U, A, rng)
            tl, ll = np.full(N, T, np.int32), np.full(N, U - 1, np.int32)
        else:
            tl, ll = ragged_lengths(N, T, U, rng, pair_without_labels=True)
            labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
        self.N, self.U, self.A, self.lib, self.add = N, U, A, _lib.lib(), case["entry"] == "align_add"
        self.lab, self.tl, self.ll = (torch.tensor(v, device=DEV) for v in (labels, tl, ll))
        self.opt = options(T, U, 0)
        self.code = {"f32": _lib.DT_F32, "f64": _lib.DT_F64, "bf16": _lib.DT_BF16, "f16": _lib.DT_F16}[case["dtype"]]
        if self.add:
            f = torch.tensor(rng.standard_normal((N, T, A)) * 1.5, dtype=torch.float32).to(dt)
            g = torch.tensor(rng.standard_normal((N, U, A)) * 1.5, dtype=torch.float32).to(dt)
            if variant == "failing":
                f[:, 0, 0] = float("nan")
            self.x = (_nan_padding(f, tl, 1).to(DEV), _nan_padding(g, ll, 2).to(DEV))
            self.nbytes = _lib.workspace_bytes_add(T, U, N)
        else:
            x = torch.tensor(acts if planted else rng.standard_normal((N, T, U, A)), dtype=torch.float32).to(dt)
            if variant == "failing":
                x[:, 0, 0, 0] = float("nan")
            for b in range(N):
                x[b, tl[b]:] = float("nan")
                x[b, :, ll[b] + 1:] = float("nan")
            self.x = (x.to(DEV),)
            self.nbytes = _lib.workspace_bytes(T, U, N, True, torch.finfo(dt).bits // 8)
        if variant == "failing":
            def failed(out):
                assert np.isnan(out["score"]).all() and (out["frames"] == -1).all(), out
            self.failed = failed

    def run(self, ws, form, scale=None):
        score = torch.full((self.N,), float("nan"), dtype=torch.float64, device=DEV)
        frames = torch.full((self.N, max(self.U - 1, 1)), -7, dtype=torch.int32, device=DEV)
        entry = self.lib.compute_rnnt_align_add if self.add else self.lib.compute_rnnt_align
        lab = self.lab.data_ptr() if self.lab.numel() else self.tl.data_ptr()
        st = entry(*(t.data_ptr() for t in self.x), lab, self.ll.data_ptr(), self.tl.data_ptr(), self.A, self.N,
                   score.data_ptr(), frames.data_ptr(), ws.data_ptr(), self.opt, self.code)
        torch.cuda.synchronize()
        assert st == 0, st
        return {"score": score.cpu().numpy(), "frames": frames.cpu().numpy()[:, :self.U - 1]}


class _Add(Problem):
    """The additive joint on a loss case of tests/joint_forms.py, as tests/test_gpu_joint_forms.py builds it: fp32 has the
    one-call entry (compute_rnnt_loss_add), every dtype _add_fwd_dt + _add_bwd_dt (fp32: _add_fwd, or _add_fwd_fastemit for a
    case with lambda, + _add_bwd); `score` is the forward entry with prepare_backward = 0.  The failing batch: a NaN row
    f[b, 0, :] in every sample (cost NaN, NaN in df).

    Not every bit of df and dg is fixed by the inputs: the correction sums sfb / sgb / sgl of the gradient GEMMs' epilogues
    (coef_kernel<float, true>, joint_sums_kernel) and the far cells (joint_far_kernel) are accumulated with float atomics, in
    the order the blocks happen to arrive.  Two runs on zero-filled workspaces can differ in the last bits, so where a run's bits
    differ from the zero-filled one's, `judge` holds it to check_loss of tests/test_gpu_joint_forms.py -- the fp64 oracle at
    that module's bounds -- instead."""

    def __init__(self, case, variant, cus):
        from tests import joint_forms as J
        from tests.gpu_support import TORCH, options
        from tests.test_gpu_joint_forms import _nan_padding, _problem, _scale
        from warprnnt_pytorch import _lib
        case = _resolve(case, cus)
        if variant == "grown":
            case = _grown(case, max_u=MAX_U)
        self.case, self.lib = case, _lib.lib()
        N, T, U, A = J.K.case_shape(case, cus)
        self.dt = TORCH[case["dtype"]]
        f, g, labels, tl, ll, blank = _problem(case, cus)
        fs, gs = (torch.tensor(v, dtype=torch.float32).to(self.dt) for v in (f, g))
        self.ref = (fs.clone(), gs.clone(), labels, tl, ll, blank)
        if variant == "failing":
            fs[:, 0] = float("nan")
            self.failed = _non_finite(list(range(N)), grads=("df",))
        self.off = dict({"f": 0, "g": 0, "df": 0, "dg": 0}, **case.get("off", {}))
        self.f = _placed(_nan_padding(fs, tl, 1), self.off["f"])
        self.g = _placed(_nan_padding(gs, ll, 2), self.off["g"])
        self.lab, self.tl, self.ll = (torch.tensor(v, device=DEV) for v in (labels, tl, ll))
        self.N, self.T, self.U, self.A = N, T, U, A
        self.nbytes = _lib.workspace_bytes_add(T, U, N)
        self.opt = options(T, U, blank)
        self.own_scale = _scale(case, N)
        self.code = {"f32": _lib.DT_F32, "bf16": _lib.DT_BF16, "f16": _lib.DT_F16}[case["dtype"]]
        self.lam = case.get("lam", 0.0)
        self.fp32 = case["entry"] != "dt"
        self.forms = ("one", "score", "two") if case["entry"] == "add" else ("score", "two")

    def judge(self, out, form, scale=None):
        from oracle import oracle as O
        from tests.test_gpu_joint_forms import check_loss
        sc = None if form == "one" else (scale if scale is not None else self.own_scale)
        check_loss(self.case, O, *self.ref, None if sc is None else np.asarray(sc, np.float64), out.get("costs"), out.get("df"),
                   out.get("dg"))

    def _fwd(self, costs, ws, prepare):
        lab = self.lab.data_ptr() if self.lab.numel() else self.tl.data_ptr()
        a = (self.f.data_ptr(), self.g.data_ptr(), lab, self.ll.data_ptr(), self.tl.data_ptr(), self.A, self.N, costs.data_ptr(),
             ws.data_ptr(), self.opt)
        if not self.fp32:
            return self.lib.compute_rnnt_loss_add_fwd_dt(*a, self.code, prepare, 0.0)
        if self.lam:
            return self.lib.compute_rnnt_loss_add_fwd_fastemit(*a, prepare, self.lam)
        return self.lib.compute_rnnt_loss_add_fwd(*a, prepare)

    def run(self, ws, form, scale=None):
        N, T, U, A = self.N, self.T, self.U, self.A
        lab = self.lab.data_ptr() if self.lab.numel() else self.tl.data_ptr()
        costs = torch.full((N,), float("nan"), device=DEV)
        df = dg = None
        if form not in ("score", "fwd"):
            df = _placed(torch.full((N, T, A), float("nan"), dtype=self.dt), self.off["df"])
            dg = _placed(torch.full((N, U, A), float("nan"), dtype=self.dt), self.off["dg"])
        sc = scale if scale is not None else self.own_scale
        t_sc = None if sc is None else torch.tensor(np.asarray(sc), dtype=torch.float32, device=DEV)
        p = (self.f.data_ptr(), self.g.data_ptr())
        st = 0
        if form == "one":
            st = self.lib.compute_rnnt_loss_add(*p, df.data_ptr(), dg.data_ptr(), lab, self.ll.data_ptr(), self.tl.data_ptr(), A, N,
                                                costs.data_ptr(), ws.data_ptr(), self.opt)
        elif form == "score":
            st = self._fwd(costs, ws, 0)
        else:
            if form != "bwd":
                st = self._fwd(costs, ws, 1)
            if form != "fwd" and st == 0:
                b = (*p, df.data_ptr(), dg.data_ptr(), None if t_sc is None else t_sc.data_ptr(), lab, self.ll.data_ptr(),
                     self.tl.data_ptr(), A, N, ws.data_ptr(), self.opt)
                st = self.lib.compute_rnnt_loss_add_bwd(*b) if self.fp32 else self.lib.compute_rnnt_loss_add_bwd_dt(*b, self.code)
        torch.cuda.synchronize()
        assert st == 0, (form, st)
        out = {} if form == "bwd" else {"costs": costs.cpu().numpy()}
        if df is not None:
            out.update(df=df.double().cpu().numpy(), dg=dg.double().cpu().numpy())
        return out


# ----------------------------------------------------------------------------- the registry
class Library:
    """One sizing function: its forms tables ({prefix: (module, cases attribute, predict attribute)}), the cases left out for
    size, and problem(case, variant, cus) with variant healthy | failing | grown."""

    fg = False                      # elements(): the cases' tensors are the additive joint's f and g

    def __init__(self, size_fn, tables, problem, left_out=()):
        self.size_fn, self.tables, self._problem, self.left_out = size_fn, tables, problem, tuple(left_out)

    def table(self, prefix):
        mod, cases, predict = self.tables[prefix]
        m = importlib.import_module("tests." + mod)
        return getattr(m, cases), getattr(m, predict)

    def all_cases(self):
        """{registry name: case} of every case of the library's tables that it takes (a table may serve two libraries)."""
        out = {}
        for prefix, (mod, _, _) in self.tables.items():
            cases, _ = self.table(prefix)
            for name, c in cases.items():
                if self.takes(prefix, c):
                    out[prefix + name] = c
        return out

    def takes(self, prefix, case):
        return True

    def cases(self):
        return {n: c for n, c in self.all_cases().items() if n not in self.left_out}

    def predicted(self, name, cus=256):
        prefix = max((p for p in self.tables if name.startswith(p)), key=len)
        cases, predict = self.table(prefix)
        c = cases[name[len(prefix):]]
        return {(c["dtype"], k) for ks in predict(c, cus).values() for k in ks}

    def problem(self, name, variant, cus):
        return self._problem(self.all_cases()[name], variant, cus)


class _MainLibrary(Library):
    """get_workspace_size: the padded and packed layouts (tests/kernel_forms.py) and compute_rnnt_align (the `align` cases of
    tests/joint_forms.py), which share its buffer."""

    def takes(self, prefix, case):
        return prefix == "" or case["entry"] == "align"


class _AddLibrary(Library):
    """get_workspace_size_add: every case of tests/joint_forms.py but the materialised alignment's."""
    fg = True

    def takes(self, prefix, case):
        return case["entry"] != "align"


def elements(case, fg=False):
    """Elements of a case's largest tensor (N as at 256 compute units); fg: the additive joint's f and g."""
    n = case.get("N", 1)
    n = 129 if isinstance(n, str) else n
    if "H" in case:                                                  # the joiner's out
        return n * case["T"] * (case["S"] if case["layout"] == 2 else case["U"]) * case["H"]
    if "mod" in case:                                                # px, py
        return n * (case["S"] + 1) * (case["T"] + 1)
    if fg or case.get("entry") == "ranges":
        return n * max(case["T"], case["U"]) * case["A"]
    width = case["A"] + (len(case["durations"]) if "durations" in case and "columns" not in case else 0)     # (TDT: A + D)
    return n * case["T"] * case.get("S", case["U"]) * width


def uncovered(lib, cus=256):
    """The leave-out rule: {left-out case: the kernels it predicts that no kept case predicts} -- every set must be empty -- and
    the left-out cases below LIMIT elements, which size does not excuse."""
    kept = set()
    for name in lib.cases():
        kept |= lib.predicted(name, cus)
    every = lib.all_cases()
    assert set(lib.left_out) <= set(every), set(lib.left_out) - set(every)
    return ({n: lib.predicted(n, cus) - kept for n in lib.left_out},
            [n for n in lib.left_out if elements(every[n], lib.fg) < LIMIT])


def _ws(attr):
    return lambda M, c, x: getattr(M, attr)().workspace_bytes(c["T"], c["U"], c["N"], _code(x))


REGISTRY = {lib.size_fn: lib for lib in (
    _MainLibrary("get_workspace_size",
                 {"": ("kernel_forms", "CASES", "predict"), "align/": ("joint_forms", "JCASES", "predict_joint")},
                 lambda c, v, cus: (_Align if c["entry"] == "align" else _Main)(c, v, cus)),
    _AddLibrary("get_workspace_size_add", {"": ("joint_forms", "JCASES", "predict_joint")},
                lambda c, v, cus: (_Align if c["entry"] == "align_add" else _Add)(c, v, cus)),
    Library("get_workspace_size_tdt", {"": ("tdt_forms", "CASES", "predict")}, _logits_library(
        "tdt", _tdt, lambda M, c, x: M._tdt().workspace_bytes(c["T"], c["U"], c["N"], len(c["durations"]), _code(x)))),
    Library("get_workspace_size_pstream", {"": ("pstream_forms", "CASES", "predict")}, _logits_library(
        "pstream", _pstream, lambda M, c, x: M._ps().workspace_bytes(c["T"], c["U"], c["S"], c["N"], _code(x)))),
    Library("get_workspace_size_kd", {"": ("kd_forms", "CASES", "predict")}, _logits_library("kd", _kd, _ws("_kd"))),
    Library("get_workspace_size_joiner", {"": ("joiner_forms", "CASES", "predict")}, _joiner_problem),
    Library("get_workspace_size_pruned", {"": ("pruned_forms", "CASES", "predict")}, _pruned_problem),
    Library("get_workspace_size_hat", {"": ("hat_forms", "CASES", "predict")}, _logits_library("hat", _hat, _ws("_hat"))),
    Library("get_workspace_size_mi", {"": ("mi_forms", "CASES", "predict")}, _mi_problem),
    Library("get_workspace_size_mono", {"": ("mono_forms", "CASES", "predict")}, _logits_library("mono", _mono, _ws("_mono")),
            left_out=("f32_u1100", "f64_u1100")),
    Library("get_workspace_size_tdt_align", {"": ("tdt_align_forms", "CASES", "predict")}, _tdt_align_problem),
    Library("get_workspace_size_ar", {"": ("ar_forms", "CASES", "predict")}, _logits_library("ar", _ar, _ws("_ar"))),
    Library("get_workspace_size_mblank", {"": ("mblank_forms", "CASES", "predict")}, _logits_library(
        "mblank", _mblank, lambda M, c, x: M._mb().workspace_bytes(c["T"], c["U"], c["N"], len(c["durations"]), _code(x)))),
    Library("get_workspace_size_delay", {"": ("delay_forms", "CASES", "predict")}, _logits_library(
        "delay", _delay, _ws("_delay"), names=("costs", "grads", "emit_frames"))),
)}


# ----------------------------------------------------------------------------- the contract of one (library, case)
def check_case(lib, name, cus):
    """Bounds, stale bytes and repeated backward for one case; module docstring.  -> the number of C-ABI forms run."""
    P = lib.problem(name, "healthy", cus)
    s1, s2 = scales(P.N, 1), scales(P.N, 2)
    runs, judged = 0, []

    def run(p, w, form, what, scale=None):
        nonlocal runs
        out = p.run(w, form, s1 if scale is None and form == "two" else scale)
        w.assert_guards("%s %s: %s, form %s" % (lib.size_fn, name, what, form))
        runs += 1
        return out

    def agree(got, want, what, form, scale=None):
        """The bits of the zero-filled run -- or, where the library sums with float atomics and they differ, its own check."""
        if P.judge is None or not differing(got, want):
            return assert_same(got, want, "%s: %s, form %s" % (name, what, form))
        assert set(got) == set(want), (what, sorted(got), sorted(want))
        P.judge(got, form, s1 if scale is None and form == "two" else scale)
        judged.append("%s, form %s: %s" % (what, form, ", ".join(differing(got, want))))

    # the zero-filled workspace: two runs agree, on a 256-byte boundary and SHIFT bytes past one; the guards hold
    zero = {}
    for form in P.forms:
        zero[form] = run(P, Workspace(P.nbytes), form, "zero-filled")
        agree(run(P, Workspace(P.nbytes), form, "zero-filled again"), zero[form], "two zero-filled runs", form)
        agree(run(P, Workspace(P.nbytes, SHIFT), form, "%d bytes past a boundary" % SHIFT), zero[form],
              "%d bytes past a 256-byte boundary" % SHIFT, form)
    # stale bytes: (a) 0xFF, (b) the same dims' failing batch, (c) other dims' healthy batch, (d) a score-only call
    bad = lib.problem(name, "failing", cus)
    big = lib.problem(name, "grown", cus)
    assert bad.nbytes == P.nbytes, (bad.nbytes, P.nbytes)
    for form in P.forms:
        agree(run(P, Workspace(P.nbytes, fill=0xFF), form, "0xFF"), zero[form], "0xFF workspace", form)
        w = Workspace(P.nbytes)
        bad.failed(run(bad, w, bad.primary, "the failing batch"))
        agree(run(P, w, form, "after the failing batch"), zero[form], "after the failing batch", form)
        w = Workspace(max(P.nbytes, big.nbytes))
        run(big, w, big.primary, "the batch of other dims")
        agree(run(P, w, form, "after other dims"), zero[form], "after a batch of other dims", form)
        if form != "score" and "score" in P.forms:
            w = Workspace(P.nbytes)
            agree(run(P, w, "score", "score-only"), zero["score"], "score-only", "score")
            agree(run(P, w, form, "after score-only"), zero[form], "after a score-only call", form)
    # repeated backward on the workspace one forward call left
    if P.halves:
        w = Workspace(P.nbytes)
        run(P, w, "fwd", "forward")
        first, second, third = (run(P, w, "bwd", "backward %d" % i, s) for i, s in enumerate((s1, s2, s1)))
        agree(third, first, "the third backward against the first (same scale)", "bwd", s1)
        agree(first, {k: v for k, v in zero["two"].items() if k in first}, "the first backward against fwd + bwd", "bwd", s1)
        fresh = run(P, Workspace(P.nbytes), "two", "fresh two-phase", s2)
        agree(second, {k: v for k, v in fresh.items() if k in second}, "the second backward against a fresh fwd + bwd", "bwd", s2)
    if judged:
        print("%s %s: judged by the module's own check where float atomics changed bits:\n  %s"
              % (lib.size_fn, name, "\n  ".join(judged)))
    return runs
