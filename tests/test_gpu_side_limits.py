"""-m gpu: every row of tests/side_limits.py.

A sliced row (N = 65536 or 65548 samples: a base block of K = 7 ragged samples, repeated) runs its library's one-call form
and its two-phase form with a per-sample scale, each under torch.profiler and each beside the same call on the base block
alone: every sliced kernel the table names for the row must have been launched ceil(N / 65535) = 2 times for each launch the
block's call made -- the second slice ran.  Every output starts as NaN (or the module's own "unset" value); every sample's
outputs are compared with the module's fp64 reference of the block, repeated, through side_limits.fold and the module's own
checker at its own bounds (tests/side_limits.py says why the largest and the smallest value of a class of samples suffice).

A trip row (elem_grid: E just over 2^24 elements, logits and gradients one element past a 16-byte boundary) must launch the
element-wise gradient kernel, whose grid-stride loop then takes a second trip, and is compared with the fp64 reference on every
in-lattice row, with exact zeros in padding, by the module's checker.

compute_rnnt_prune_ranges_add refuses N > 65535 (include/rnnt_pruned.h): the refusal is tested, nothing written."""
import importlib
import time

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import side_limits as SL
from tests import ws_contract as W
from tests.gpu_support import CODE, DEV, dev, options, place, profiled

pytestmark = pytest.mark.gpu


def _module(lib):
    return importlib.import_module("tests.test_gpu_" + lib)


def _need(nbytes):
    free = torch.cuda.mem_get_info(0)[0]
    if free < nbytes:
        print("SKIPPED: %d bytes of device memory free, the row needs %d" % (free, nbytes))
        pytest.skip("device memory is short")


def _is_batch(a):
    return (isinstance(a, np.ndarray) or torch.is_tensor(a)) and a.ndim >= 1 and a.shape[0] == SL.K


def _tiled(items, n, device=False):
    out = []
    for a in items:
        if _is_batch(a):
            a = SL.tile(a, n)
            if device and torch.is_tensor(a):
                a = a.to(DEV)
        out.append(a)
    return out


def _profiled(fn, wanted):
    """profiled(fn); a session that did not record every one of the `wanted` kernels at least once runs once more (a profiler
    session now and then records no device event at all, or loses the first ones) and is judged as the first would have been.
    A kernel that is never launched is missing from the second session too, and a slice that is not launched leaves its
    kernel with the count of one slice, not with none."""
    out, names = profiled(fn)
    if not all(k in names for k in wanted):
        out, names = profiled(fn)
    return out, names


def _slice_faults(row, names_block, names_full, form):
    want = SL.kernels(row, G.cus())
    assert want
    bad = []
    for k in sorted(want):
        per_call = names_block.count(k)
        if per_call < 1:
            bad.append((row["name"], form, k, "not launched for the base block", sorted(set(names_block))))
        elif names_full.count(k) != SL.slices(row) * per_call:
            bad.append((row["name"], form, k, names_full.count(k), per_call))
    return bad


def _sliced_calls(row, form, call_block, call_full):
    """The call on the base block and on the full batch, each under the profiler -> what the full call returned.  Every
    sliced kernel of the row: slices(row) launches in the full call for each launch in the block's.  Which kernels a call
    launches is a function of its arguments alone, what a profiler session records is not (it now and then loses events):
    counts that do not fit are taken once more, from two new sessions, and those must fit."""
    wanted = SL.kernels(row, G.cus())
    for attempt in (0, 1):
        out_b, names_b = _profiled(call_block, wanted)
        out, names = _profiled(call_full, wanted)
        bad = _slice_faults(row, names_b, names, form)
        if not bad:
            return out_b, out
        print("%s, form %s: launch counts of session %d: %s" % (row["name"], form, attempt, bad))
    raise AssertionError(bad)


# ----------------------------------------------------------------------------- the losses on one logits tensor
# library -> (builder of tests/ws_contract.py, (rest, kw) -> the reference's arguments, (case, rest, kw) -> the checker's
# arguments behind the mask); rest and kw as the builder returns them, on K or on PERIOD samples
LOGITS = {
    "hat": (W._hat, lambda r, kw: (r, kw), lambda c, r, kw: (r[0], r[2], kw["blank"])),
    "tdt": (W._tdt, lambda r, kw: (r, kw), lambda c, r, kw: (r[0], r[2], c["A"])),
    "mblank": (W._mblank, lambda r, kw: (r, kw), lambda c, r, kw: (r[0], r[2], kw["blank"], r[3])),
    "ar": (W._ar, lambda r, kw: (r, kw), lambda c, r, kw: (r[0], r[2], kw["blank"])),
    "delay": (W._delay, lambda r, kw: (r, kw), lambda c, r, kw: (r[0], r[2], kw["blank"])),
    "mono": (W._mono, lambda r, kw: (r, kw), lambda c, r, kw: (r[0], r[2], kw["blank"])),
    "pstream": (W._pstream, lambda r, kw: (r[:4], kw), lambda c, r, kw: (r[0], r[1], r[3], kw["blank"], kw["typ"], r[4])),
    "pruned": (W._pruned, lambda r, kw: (r[:4], {}), lambda c, r, kw: (r[0], r[3], r[2])),
}


def _logits_problem(row, case):
    """The block of a row: (M, x, rest, kw, mask, check) with check(outs, scale) the module's checker against the reference of
    the block repeated to PERIOD samples."""
    lib = row["lib"]
    M = _module(lib)
    dtype = row["dtype"]
    if lib == "kd":
        z, rest, kw, mask = W._kd(M, case)
        z28, rest28 = SL.tile(z, SL.PERIOD), _tiled(rest, SL.PERIOD)

        def check(o, scale):
            ref = M.Ref(z28, *rest28, kw["blank"], kw["mode"], kw["tau"], weights=scale)
            M._check(dtype, o["costs"], o.get("grads"), ref, what=row["name"])
        return M, z, rest, kw, mask, check
    build, ref_args, tail = LOGITS[lib]
    x, rest, kw, mask = build(M, case)
    ra, rk = ref_args(list(rest), kw)
    rc, rg = M._reference(x, *ra, **rk)
    rc28, rg28, mask28 = SL.tile(rc, SL.PERIOD), SL.tile(rg, SL.PERIOD), SL.tile(mask, SL.PERIOD)
    rest28 = _tiled(rest, SL.PERIOD)
    emit28 = SL.tile(M._emit_reference(x, *ra, **rk), SL.PERIOD) if lib == "delay" else None

    def check(o, scale):
        M._check(dtype, o["costs"], o.get("grads"), rc28, rg28, mask28, *tail(case, rest28, kw), scale=scale, what=row["name"])
        if emit28 is not None:
            M._check_emit(dtype, o["emit"], emit28, rest28[1], rest28[2], what=row["name"])
    return M, x, rest, kw, mask, check


def _run_logits(row):
    case = SL.block_case(row)
    N = row["N"]
    M, x, rest, kw, _, check = _logits_problem(row, case)
    _need(6 * N * x[0].numel() * 8)
    xb, restb = x.to(DEV), _tiled(rest, SL.K, device=True)
    xn, restn = SL.tile(x, N).to(DEV), _tiled(rest, N, device=True)
    for form, scaled in (("one", False), ("two", True)):
        (stb, *_), (st, *out) = _sliced_calls(
            row, form, lambda: M.call(xb, *restb, **kw, form=form, scale=SL.scale_of(SL.K) if scaled else None),
            lambda: M.call(xn, *restn, **kw, form=form, scale=SL.scale_of(N) if scaled else None))
        assert stb == 0 and st == 0
        outs = dict(zip(("costs", "grads", "emit"), out))
        SL.check_folded(outs, check, scaled)


# ----------------------------------------------------------------------------- mi: px / py edge log-probs, two gradients
def _run_mi(row):
    M = _module("mi")
    case = SL.block_case(row)
    N, dtype = row["N"], row["dtype"]
    px, py, bd, mx, my = M._table_problem(case)
    _need(8 * N * (px[0].numel() + py[0].numel()) * 8)
    px28, py28, bd28 = SL.tile(px, SL.PERIOD), SL.tile(py, SL.PERIOD), SL.tile(bd, SL.PERIOD)
    mx28, my28 = SL.tile(mx, SL.PERIOD), SL.tile(my, SL.PERIOD)

    def check(o, scale):
        rsc, rgx, rgy = M._reference(px28, py28, bd28, weights=scale)
        M._check(dtype, o["scores"], o["px_grad"], o["py_grad"], rsc, rgx, rgy, mx28, my28, scale=scale, what=row["name"])
    xb, yb = px.to(DEV), py.to(DEV)
    xn, yn, bdn = SL.tile(px, N).to(DEV), SL.tile(py, N).to(DEV), SL.tile(bd, N)
    for form, scaled in (("one", False), ("two", True)):
        (stb, *_), (st, *out) = _sliced_calls(row, form, lambda: M.call(xb, yb, bd, form, SL.scale_of(SL.K) if scaled else None),
                                              lambda: M.call(xn, yn, bdn, form, SL.scale_of(N) if scaled else None))
        assert stb == 0 and st == 0
        SL.check_folded(dict(zip(("scores", "px_grad", "py_grad"), out)), check, scaled)


# ----------------------------------------------------------------------------- bestpath: scores, frames, back, indicators
def _run_bestpath(row):
    M = _module("bestpath")
    case = SL.block_case(row)
    N, mod = row["N"], row["mod"]
    px, py, bd, _, _ = M._table_problem(case)
    _need(8 * N * (px[0].numel() + py[0].numel()) * 8)
    px28, py28, bd28 = SL.tile(px, SL.PERIOD), SL.tile(py, SL.PERIOD), SL.tile(bd, SL.PERIOD)
    ref28 = M._reference(px28, py28, bd28, mod)
    xb, yb = px.to(DEV), py.to(DEV)
    xn, yn, bdn = SL.tile(px, N).to(DEV), SL.tile(py, N).to(DEV), SL.tile(bd, N)

    def check_for(scale28):
        def check(o, _scale):
            got = dict(o, st=0)
            M._same(got, ref28, row["name"])
            M._check_edges(got, px28, py28, bd28, mod, scale=scale28, what=row["name"])
        return check
    # the one call with every output, then the second entry on its frames and scores with a per-sample scale
    got_b, got = _sliced_calls(row, "all", lambda: M.call(xb, yb, bd, "all"), lambda: M.call(xn, yn, bdn, "all"))
    assert got_b["st"] == 0 and got["st"] == 0
    keys = ("scores", "frames", "back", "ex", "ey")
    SL.check_folded({k: got[k] for k in keys}, check_for(None), False)
    edges_b, edges = _sliced_calls(row, "edges", lambda: M.call(xb, yb, bd, "edges", SL.scale_of(SL.K), prev=got_b),
                                   lambda: M.call(xn, yn, bdn, "edges", SL.scale_of(N), prev=got))
    assert edges_b["st"] == 0 and edges["st"] == 0
    SL.check_folded({k: edges[k] for k in keys}, check_for(SL.scale_of(SL.PERIOD)), True)


# ----------------------------------------------------------------------------- tdt_align: score, frames, durations
def _run_tdt_align(row):
    M = _module("tdt_align")
    case = SL.block_case(row)
    N, dtype, durs = row["N"], row["dtype"], row["durations"]
    x, labels, tl, ll, _ = M._problem(case["name"], dtype, SL.K, case["T"], case["U"], case["A"], durs)
    _need(4 * N * x[0].numel() * 8)
    x28, lab28, tl28, ll28 = (SL.tile(a, SL.PERIOD) for a in (x, labels, tl, ll))
    xr, ref = M.reference(x28, lab28, tl28, ll28, durs)
    fin = [b for b in range(SL.PERIOD) if np.isfinite(ref[0][b])]
    assert any(ll28[b] > 0 for b in fin), (row["name"], ref[0], ll28)

    def check(o, _scale):
        got = (o["score"], o["frames"], o["durs"])
        for b in set(range(SL.PERIOD)) - set(fin):
            assert got[0][b] == -np.inf and (got[1][b] == -1).all() and (got[2][b] == -1).all(), (row["name"], b)
        M.check(dtype, xr, lab28, tl28, ll28, durs, 0, 0.0, got, ref, row["name"], fin)
    xb = x.to(DEV)
    xn, labn, tln, lln = SL.tile(x, N).to(DEV), SL.tile(labels, N), SL.tile(tl, N), SL.tile(ll, N)
    (stb, *_), (st, *out) = _sliced_calls(row, "one", lambda: M.call(xb, labels, tl, ll, durs),
                                          lambda: M.call(xn, labn, tln, lln, durs))
    assert stb == 0 and st == 0
    outs = dict(zip(("score", "frames", "durs"), out))
    # the labelling is a function of a sample's data alone: every copy of a block position gives the same one
    for k in ("frames", "durs"):
        hi, lo = SL.fold(outs[k], k)
        assert np.array_equal(hi, lo), (row["name"], k, "copies of one sample are labelled differently")
    SL.check_folded(outs, check, False)


# ----------------------------------------------------------------------------- joiner: out, df, dg, flags
def _fold_t(t, period):
    """side_limits.fold on the device, in the tensor's own type, over a first axis of `period` rows per PERIOD samples."""
    full, rest = divmod(t.shape[0], period)
    assert full >= 1
    body = t[:full * period].view((full, period) + tuple(t.shape[1:]))
    hi, lo = body.amax(0), body.amin(0)
    nans = torch.isnan(body).sum(0)
    assert bool(((nans == 0) | (nans == full)).all()), "NaN in some samples of a class and not in others"
    tail = t[full * period:]
    assert torch.equal(torch.isnan(tail), nans[:rest] == full)
    hi[:rest], lo[:rest] = torch.maximum(hi[:rest], tail), torch.minimum(lo[:rest], tail)
    return hi, lo


def _run_joiner(row):
    """No sample loop here: joiner_prep_kernel takes N on grid.x, and past 65535 samples the backward call takes
    joiner_df_kernel and joiner_dg_kernel (jn_plan: the single pass has N on grid.y).  Each predicted kernel is launched
    once, no other; out, df, dg of every sample against the module's checks on PERIOD samples; the flags all zero."""
    M = _module("joiner")
    F = SL.forms_of("joiner")
    case = SL.block_case(row)
    N, dtype, lay = row["N"], row["dtype"], row["layout"]
    rng, f, g = M._fg(case["name"], dtype, SL.K, case["T"], case["U"], case["H"])
    tl, ll = F.lengths(case, rng)
    ranges = F.ranges(case, rng) if lay == 2 else None

    def problem(n):
        return M.Problem(dtype, lay, row["act"], n, case["T"], case["U"], case["H"], case["S"], SL.tile(tl, n), SL.tile(ll, n),
                         None if ranges is None else SL.tile(ranges, n))
    pb, pp, pn = problem(SL.K), problem(SL.PERIOD), problem(N)
    dout = M._dout(pb, rng)
    rows_of = lambda p: p.shape[0]                                                           # noqa: E731

    def both(p):
        n = p.N
        out = p.fwd(SL.tile(f, n), SL.tile(g, n))
        o_nan, d_nan = M.poisoned(p, out, SL.tile(dout, rows_of(p)))
        return (out,) + tuple(p.bwd(o_nan, d_nan))
    want = F.predict(SL.full_case(row))
    assert set(want) >= {"fwd", "df", "dg"} and "bwd" not in want
    wanted = SL.kernels(row)
    (out, df, dg), names = _profiled(lambda: both(pn), wanted)
    M.assert_stages(row["name"], M.stages_seen(names, F.stage_of, F.STAGES), want)
    for k in wanted:                                                   # (the pruned layout: prep in both calls)
        assert names.count(k) == (2 if "prep_kernel" in k else 1), (row["name"], k, names.count(k))
    if lay == 2:
        assert not pn.flags().any(), (row["name"], "a flag is raised")
    f28, g28 = SL.tile(f, SL.PERIOD), SL.tile(g, SL.PERIOD)
    per = rows_of(pp)
    o_hi, o_lo = _fold_t(out, per)
    assert torch.equal(M._bits(o_hi), M._bits(o_lo)), (row["name"], "copies of one sample differ in out")
    M.check_forward(pp, f28, g28, o_hi, row["name"])
    o_nan, d_nan = M.poisoned(pp, o_hi, SL.tile(dout, per))
    (df_hi, df_lo), (dg_hi, dg_lo) = _fold_t(df, SL.PERIOD), _fold_t(dg, SL.PERIOD)
    M.check_backward(pp, o_nan, d_nan, df_hi, dg_hi, row["name"])
    M.check_backward(pp, o_nan, d_nan, df_lo, dg_lo, row["name"])


RUN = {"mi": _run_mi, "bestpath": _run_bestpath, "tdt_align": _run_tdt_align, "joiner": _run_joiner}


@pytest.mark.parametrize("name", sorted(SL.ROWS))
def test_sliced_row(name):
    row = SL.ROWS[name]
    t0 = time.time()
    RUN.get(row["lib"], _run_logits)(row)
    print("%s: %.1f s" % (name, time.time() - t0))


# ----------------------------------------------------------------------------- the second trip of the element-wise gradient
@pytest.mark.parametrize("name", sorted(SL.TRIP_ROWS))
def test_elem_grid_second_trip(name):
    row = SL.TRIP_ROWS[name]
    t0 = time.time()
    case = SL.full_case(row)
    M, x, rest, kw, mask = _trip_problem(row, case)
    off, dtype = row["off"], row["dtype"]
    _need(8 * x.numel() * 8)
    tl, ll = (rest[2], rest[3]) if row["lib"] == "kd" else (rest[1], rest[2])
    assert (tl == row["T"]).all() and (ll == row["U"] - 1).all()       # every sample full length
    xd = place(x.to(DEV), off, x.dtype)
    gd = place(torch.full_like(x, float("nan")).to(DEV), off, x.dtype)
    restd = [place(a.to(DEV), off + row.get("toff", 0), a.dtype) if torch.is_tensor(a) else a for a in rest]
    kernel = SL.trip_kernel(row)
    (st, c, g), names = _profiled(lambda: M.call(xd, *restd, **kw, form="one", grads=gd), {kernel})
    assert st == 0
    assert names.count(kernel) == 1 and SL.trips(row) == 2, (name, kernel, sorted(set(names)))
    b, r, col = SL.trip_boundary(row)
    assert b == row["N"] - 1 and mask.reshape(row["N"], -1)[b, r]
    _trip_check(row, M, x, rest, kw, mask, case, c, g)
    print("%s: %.1f s" % (name, time.time() - t0))


def _trip_problem(row, case):
    lib = row["lib"]
    M = _module(lib)
    build = W._kd if lib == "kd" else LOGITS[lib][0]
    x, rest, kw, mask = build(M, case)
    return M, x, rest, kw, mask


def _trip_check(row, M, x, rest, kw, mask, case, c, g):
    lib, dtype = row["lib"], row["dtype"]
    if lib == "kd":
        M._check(dtype, c, g, M.Ref(x, *rest, kw["blank"], kw["mode"], kw["tau"]), what=row["name"])
        return
    _, ref_args, tail = LOGITS[lib]
    ra, rk = ref_args(list(rest), kw)
    rc, rg = M._reference(x, *ra, **rk)
    M._check(dtype, c, g, rc, rg, mask, *tail(case, list(rest), kw), what=row["name"])


# ----------------------------------------------------------------------------- the second trip of the logprobs grid
@pytest.mark.parametrize("name", sorted(SL.LP_ROWS))
def test_logprobs_second_trip(name):
    """2^28 + 8 rows of 2 to 8 columns, joint form: logprobs_edges_kernel (2^28 cells per trip) and logprobs_grad_kernel
    (2^27 or 2^28 rows per trip) each take a second trip.  As tests/test_gpu_logprobs.py's test past 2^31 elements, at its
    bounds: the first and the last rows and the rows either side of every trip boundary against the reference; over the whole
    tensors, the finite-or-not pattern of lse, px, py and dlogits equals that of an fp64 torch evaluation on the device."""
    M = _module("logprobs")
    F = SL.forms_of("logprobs")
    row = SL.LP_ROWS[name]
    t0 = time.time()
    dtype, B, T, U, C = row["dtype"], row["B"], row["T"], row["U"], row["C"]
    assert B == 1 and U == 2
    _need(SL.lp_bytes(row) + (1 << 30))
    rows = B * T * U
    lat = torch.float64 if dtype == "f64" else torch.float32
    z = torch.empty((B, T, U, C), dtype=G.TORCH[dtype], device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(SL.row_seed(row))
    flat = z.view(-1)
    for at in range(0, flat.numel(), 1 << 28):
        flat[at:at + (1 << 28)].normal_(0, 2, generator=gen)
    s, blank = 0, C - 1
    sym = torch.full((B, U - 1), s, dtype=torch.int32, device=DEV)
    px = torch.full((B, U - 1, T + 1), float("nan"), dtype=lat, device=DEV)
    py = torch.full((B, U, T), float("nan"), dtype=lat, device=DEV)
    lse = torch.full((B, T, U), float("nan"), dtype=lat, device=DEV)
    gx = torch.randn(px.shape, dtype=lat, device=DEV, generator=gen)
    gy = torch.randn(py.shape, dtype=lat, device=DEV, generator=gen)
    dz = torch.full_like(z, float("nan"))
    lib, opt, code = M._lp().lib(), options(T, U, blank), CODE[dtype]

    def run():
        st = lib.compute_rnnt_logprobs_fwd(z.data_ptr(), sym.data_ptr(), None, 0, None, 0, T, U, C, B, px.data_ptr(), py.data_ptr(),
                                           lse.data_ptr(), opt, code)
        assert st == 0
        st = lib.compute_rnnt_logprobs_bwd(z.data_ptr(), lse.data_ptr(), sym.data_ptr(), None, 0, None, 0, gx.data_ptr(),
                                           gy.data_ptr(), None, T, U, C, B, dz.data_ptr(), opt, code)
        assert st == 0
        torch.cuda.synchronize()
    want = F.predict(row)
    _, names = _profiled(run, want["edges"] | want["grad"])
    for stage in ("lse", "edges", "grad"):
        (k,) = want[stage]
        assert names.count(k) == 1, (name, k, names.count(k), sorted(set(names)))
    trips = SL.lp_trips(row)
    assert min(trips.values()) >= 2
    # the rows either side of every trip boundary: of the gradient's rows, and of the edges kernel's cells (t fastest)
    check = {0, 1, rows - 2, rows - 1}
    (_, per_g), (_, per_e) = SL.lp_work(row)["logprobs_grad_kernel"], SL.lp_work(row)["logprobs_edges_kernel"]
    for i in range(1, trips["logprobs_grad_kernel"]):
        check |= {i * SL.LP_CAP * per_g - 1, i * SL.LP_CAP * per_g}
    for i in range(1, trips["logprobs_edges_kernel"]):
        for cell in (i * SL.LP_CAP * per_e - 1, i * SL.LP_CAP * per_e):
            u_, t_ = divmod(cell, T + 1)
            if t_ < T:
                check.add(t_ * U + u_)
    u = M.U_LAT[dtype]
    for r in sorted(check):
        t, k = divmod(r, U)
        zr = z[0, t, k].double().cpu().numpy()
        ref_l = M.R.row_lse(zr)
        base = (C - 1) + 2 * np.abs(zr - zr.max()).max() + abs(ref_l) + M.K_FN
        assert abs(lse[0, t, k].item() - ref_l) <= u * base, r
        assert abs(py[0, k, t].item() - (zr[blank] - ref_l)) <= u * (base + abs(zr[blank])), r
        g_x = gx[0, 0, t].item() if k == 0 else 0.0
        g_y, l = gy[0, k, t].item(), float(lse[0, t, k].item())
        if k == 0:
            assert abs(px[0, 0, t].item() - (zr[s] - ref_l)) <= u * (base + abs(zr[s])), r
        coef = -g_x - g_y
        ref = coef * np.exp(zr - l)
        ref[blank] += g_y
        if k == 0:
            ref[s] += g_x
        bound = u * (abs(coef) * np.exp(zr - l) * (np.abs(zr - l) + M.K_FN) + 2 * np.abs(ref)) + M.store_rounding(ref, dtype)
        assert (np.abs(dz[0, t, k].double().cpu().numpy() - ref) <= bound).all(), r
    # the whole tensors: finite or not, against fp64 torch on the device, in slabs of frames
    assert bool((px[:, :, T] == -float("inf")).all())
    step = 1 << 23
    for a in range(0, T, step):
        b = min(a + step, T)
        zs = z[0, a:b].double()
        ls = torch.logsumexp(zs, -1)                                                   # (frames, U)
        assert torch.equal(torch.isfinite(lse[0, a:b]), torch.isfinite(ls)), (name, "lse", a)
        assert torch.equal(torch.isfinite(py[0, :, a:b]), torch.isfinite(zs[..., blank] - ls).T), (name, "py", a)
        assert torch.equal(torch.isfinite(px[0, 0, a:b]), torch.isfinite(zs[:, 0, s] - ls[:, 0])), (name, "px", a)
        gys = gy[0, :, a:b].T.double()
        gxs = torch.zeros_like(gys)
        gxs[:, 0] = gx[0, 0, a:b].double()
        ref = (-gxs - gys)[..., None] * torch.exp(zs - ls[..., None])
        ref[..., blank] += gys
        ref[:, 0, s] += gxs[:, 0]
        assert torch.equal(torch.isfinite(dz[0, a:b]), torch.isfinite(ref)), (name, "dlogits", a)
        assert bool(torch.isfinite(ref).all())
        del zs, ls, ref, gys, gxs
    print("%s: %.1f s" % (name, time.time() - t0))


# ----------------------------------------------------------------------------- the second trip of the joiner's row grid
@pytest.mark.parametrize("name", sorted(SL.JN_ROWS))
def test_joiner_second_trip(name):
    """N = 65537 full-length samples, padded layout: 2^28 + 69633 rows of out and of df (T = 4097, U = 1) or of dg (T = 1,
    U = 4097), one thread along a row, so joiner_fwd_kernel and joiner_df_kernel or joiner_dg_kernel take a second trip of
    their grid-stride loops.  out: every bit of the whole tensor against torch's own act(f + g) in the storage type (the
    module's rule for identity and relu).  df, dg: the first and the last rows and the rows either side of the trip boundary
    against the fp64 reference on the stored out and dout at the module's bound (tests/test_gpu_joiner.py, check_backward);
    over the whole tensors the finite-or-not pattern of an fp64 torch evaluation on the device."""
    M = _module("joiner")
    F = SL.forms_of("joiner")
    row = SL.JN_ROWS[name]
    t0 = time.time()
    dtype, act, N, T, U, H = row["dtype"], row["act"], row["N"], row["T"], row["U"], row["H"]
    assert act in ("identity", "relu")
    _need(SL.jn_bytes(row) + (1 << 30))
    dt = G.TORCH[dtype]
    gen = torch.Generator(device=DEV).manual_seed(SL.row_seed(row))

    def randn(shape):
        t = torch.empty(shape, dtype=dt, device=DEV)
        flat = t.view(-1)
        for at in range(0, flat.numel(), 1 << 28):
            flat[at:at + (1 << 28)].normal_(0, 1, generator=gen)
        return t
    f, g, dout = randn((N, T, H)), randn((N, U, H)), randn((N, T, U, H))
    out = torch.full((N, T, U, H), float("nan"), dtype=dt, device=DEV)
    df = torch.full((N, T, H), float("nan"), dtype=dt, device=DEV)
    dg = torch.full((N, U, H), float("nan"), dtype=dt, device=DEV)
    jn = M._jn()
    ws = torch.empty(jn.workspace_bytes(T, U, 0, H, N, 0, CODE[dtype]), dtype=torch.uint8, device=DEV)
    tail = (0, M.R.ACTS.index(act), None, 0, None, None, None, T, U, H, N, ws.data_ptr(), options(T, U), CODE[dtype])

    def run():
        assert jn.lib().compute_rnnt_joiner_fwd(f.data_ptr(), g.data_ptr(), out.data_ptr(), *tail) == 0
        assert jn.lib().compute_rnnt_joiner_bwd(None if act == "identity" else out.data_ptr(), dout.data_ptr(), df.data_ptr(),
                                                dg.data_ptr(), *tail) == 0
        torch.cuda.synchronize()
    case = {k: v for k, v in row.items() if k not in ("lib", "grid", "heavy")}
    want = F.predict(case)
    every = {k for ks in want.values() for k in ks}
    _, names = _profiled(run, every)
    M.assert_stages(name, M.stages_seen(names, F.stage_of, F.STAGES), want)
    for k in every:
        assert names.count(k) == 1, (name, k, names.count(k))
    trips, work = SL.jn_trips(row), SL.jn_work(row)
    assert len(SL.jn_kernels(row)) == 2
    # forward: the whole tensor, bit for bit
    mine = torch.empty_like(out)
    step = 4096
    for a in range(0, N, step):
        b = min(a + step, N)
        mine[a:b] = M.TORCH_ACT[act](f[a:b, :, None] + g[a:b, None])
    assert torch.equal(M._bits(out), M._bits(mine)), (name, "out is not bit-exact against torch")
    del mine
    # backward: sampled rows at the module's bound
    def term(d, o):
        return M.R.term(M._np(d), M._np(o), act)

    def close(got, e, what):
        ref, a, n = e.sum(0), np.abs(e).sum(0), e.shape[0]
        bound = max(n - 1, 0) * M.U_SUM[dtype] * a + M.store_rounding(ref, dtype)
        assert (np.abs(M._np(got) - ref) <= bound).all(), (name, what, M._np(got), ref, bound)
    for kern, rows_of, tensor in (("joiner_df_kernel", N * T, "df"), ("joiner_dg_kernel", N * U, "dg")):
        per = work[kern][1]
        check = {0, 1, rows_of - 2, rows_of - 1}
        for i in range(1, trips[kern]):
            check |= {i * SL.JN_CAP * per - 1, i * SL.JN_CAP * per}
        for r in sorted(check):
            if tensor == "df":
                b, t = divmod(r, T)
                close(df[b, t], term(dout[b, t], out[b, t]), ("df", b, t))
            else:
                b, u_ = divmod(r, U)
                close(dg[b, u_], term(dout[b, :, u_], out[b, :, u_]), ("dg", b, u_))
    # the whole tensors: finite or not, against fp64 torch on the device
    for a in range(0, N, step):
        b = min(a + step, N)
        e = dout[a:b].double()
        if act == "relu":
            e = e * (out[a:b] > 0)
        assert torch.equal(torch.isfinite(df[a:b]), torch.isfinite(e.sum(2))), (name, "df", a)
        assert torch.equal(torch.isfinite(dg[a:b]), torch.isfinite(e.sum(1))), (name, "dg", a)
        assert bool(torch.isfinite(e).all())
        del e
    print("%s: %.1f s" % (name, time.time() - t0))


# ----------------------------------------------------------------------------- the documented limit
def test_prune_ranges_refuses_more_than_65535_samples():
    """compute_rnnt_prune_ranges_add: N = 65536 -> RNNT_STATUS_INVALID_VALUE, the ranges untouched; N = 65535 is taken."""
    M = _module("pruned")
    T, U, A, S = 2, 3, 4, 2
    for N, want in ((SL.GRID_SAMPLES + 1, 2), (SL.GRID_SAMPLES, 0)):
        rng = np.random.default_rng(N)
        f = torch.tensor(rng.standard_normal((N, T, A)), dtype=torch.float32, device=DEV)
        g = torch.tensor(rng.standard_normal((N, U, A)), dtype=torch.float32, device=DEV)
        lab, ttl, tll = dev(rng.integers(1, A, size=(N, U - 1)).astype(np.int32), np.full(N, T, np.int32),
                            np.full(N, U - 1, np.int32))
        out = torch.full((N, T), -7, dtype=torch.int32, device=DEV)
        ws = torch.empty(M._pl().workspace_bytes(T, U, N, CODE["f32"]), dtype=torch.uint8, device=DEV)
        st = M._pl().lib().compute_rnnt_prune_ranges_add(f.data_ptr(), g.data_ptr(), lab.data_ptr(), tll.data_ptr(),
                                                         ttl.data_ptr(), A, N, S, out.data_ptr(), ws.data_ptr(), options(T, U),
                                                         CODE["f32"])
        torch.cuda.synchronize()
        assert st == want, (N, st)
        if want:
            assert bool((out == -7).all())
        else:
            assert bool(((out >= 0) & (out <= U - 1)).all())
