"""-m gpu: the pruned RNN-T loss and the prune ranges (include/rnnt_pruned.h, libwarprnnt_pruned.so).

Every case of tests/pruned_forms.py runs through the C-ABI under torch.profiler: exactly the kernels its release rules predict
run, stage by stage.  Loss cases are compared with the fp64 autograd reference of tests/pruned_ref.py at the per-dtype bounds
of oracle.grad_bound; ragged lengths (one sample with T_b = 1, one with L_b = 0), NaN in every padding row (never read) and
gradient buffers that start as NaN (padding must come back as exact zeros).  Ranges cases are checked against the invariants of
the rule.  Then the call forms, the reduction to compute_rnnt_loss_async, the impossible and invalid windows, the ranges
against the numpy rule, and the recipe end to end."""
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import gpu_support as G
from tests import pruned_forms as P
from tests import pruned_ref as R
from tests.gpu_support import (CODE, DEV, NAME, TORCH, assert_every_row_reached, assert_stages, call_forms, check, dev,
                               options, place, profiled, ragged_lengths, stages_seen)

pytestmark = pytest.mark.gpu


def _pl():
    from warprnnt_pytorch import pruned
    return pruned


def _windows(N, T, S, tl, ll, rng):
    """Window starts (N, T).  Every sample whose windows can hold a path gets the rule's windows on a random occupancy (a path
    through them exists), odd samples the rule's windows for S - 1 (the same guarantee, windows that may run past L_b); when
    N >= 4 the last sample is the designated one without a path: a valid start L_b > 0 in every frame, (0, 0) outside its
    window.  Samples whose windows cannot hold a path (L_b > T_b (S - 1)) get random starts in [0, L_b]."""
    r = np.zeros((N, T), np.int32)
    nopath = N - 1 if N >= 4 else -1
    if nopath >= 0 and ll[nopath] == 0 and ll.max() > 0:
        ll[nopath] = 1
    for b in range(N):
        Tb, L = int(tl[b]), int(ll[b])
        if b == nopath and L > 0:
            r[b, :Tb] = L
        elif S >= 3 and b % 2 == 1 and L <= Tb * (S - 2):
            r[b, :Tb] = R.ranges_rule(rng.random((Tb, L + 1)), Tb, L, S - 1)
        elif S >= 2 and L <= Tb * (S - 1):
            r[b, :Tb] = R.ranges_rule(rng.random((Tb, L + 1)), Tb, L, S)
        elif S == 1 and L == 0:
            r[b, :Tb] = 0
        else:
            r[b, :Tb] = rng.integers(0, L + 1, size=Tb)
    return r


def _assert_real_lattice(c, tl, ll, ranges, S, what):
    """Not only +inf: a sample with labels (L_b > 0) and a path through its windows came out finite, and every sample's
    finiteness is what its windows say."""
    for b in range(len(c)):
        assert bool(np.isfinite(c[b])) == R.has_path(ranges[b], int(tl[b]), int(ll[b]), S), (what, b, c[b])
    if S >= 2:
        assert any(np.isfinite(c[b]) and ll[b] > 0 for b in range(len(c))), (what, c, ll)


def _problem(name, dtype, N, T, U, A, S, rng=None, lengths=None):
    rng = rng or np.random.default_rng(zlib.crc32(name.encode()))
    tl, ll = lengths if lengths is not None else ragged_lengths(N, T, U, rng)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32) if A > 1 else np.zeros((N, U - 1), np.int32)
    ranges = _windows(N, T, S, tl, ll, rng)
    x = torch.tensor(rng.standard_normal((N, T, S, A)) * 2.0, dtype=torch.float32).to(TORCH[dtype])
    mask = R.in_lattice_mask((N, T, S), ranges, tl, ll)
    x[torch.tensor(~mask)] = float("nan")
    return x, labels, tl, ll, ranges, mask


def call(x, labels, tl, ll, ranges, S, U, form="one", scale=None, grads=None, blank=0, stream=None, ws=None):
    """One C-ABI call form -> (status, costs, grads or None).  form: one | two | inplace | score | host."""
    pl = _pl()
    N, T, A = x.shape[0], x.shape[1], x.shape[3]
    code = CODE[NAME[x.dtype]]
    lab, ttl, tll, tr = dev(labels if labels.size else np.zeros((N, 1), np.int32), tl, ll, ranges)
    opt = options(T, U, blank, stream)
    lib = pl.lib()
    lens = (lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A, N)
    return call_forms(
        x, form,
        lambda gp, costs, ws: lib.compute_rnnt_loss_pruned(x.data_ptr(), gp, tr.data_ptr(), S, *lens, costs, ws, opt, code),
        lambda costs, ws: lib.compute_rnnt_loss_pruned_fwd(x.data_ptr(), tr.data_ptr(), S, *lens, costs, ws, opt, code, 1),
        lambda gp, sc, ws: lib.compute_rnnt_loss_pruned_bwd(x.data_ptr(), gp, sc, S, A, N, ws, opt, code),
        pl.workspace_bytes(T, U, N, code), scale, grads, stream, ws)


def _reference(x, labels, tl, ll, ranges, weights=None):
    xr = torch.nan_to_num(x.double(), nan=0.0).cpu().numpy()
    return R.pruned_autograd(xr, labels, ranges, tl, ll, 0, weights)


def _mag(ref, labels, ranges, ll, blank=0):
    """The size of the terms of every gradient element: |ref|, and for the blank and label columns the row's |ref| sum."""
    mag = np.abs(ref).copy()
    rs = np.abs(ref).sum(-1)
    N, T, S, _ = ref.shape
    mag[..., blank] = np.maximum(mag[..., blank], rs)
    for b in range(N):
        for t in range(T):
            for k in range(S):
                u = int(ranges[b, t]) + k
                if u < int(ll[b]):
                    lab = int(labels[b, u])
                    mag[b, t, k, lab] = max(mag[b, t, k, lab], rs[b, t, k])
    return mag


def _check(dtype, got_c, got_g, ref_c, ref_g, mask, labels, ranges, ll, scale=None, what=""):
    check(dtype, got_c, got_g, ref_c, ref_g, mask,
          lambda ref, b: _mag(ref, labels[b:b + 1], ranges[b:b + 1], ll[b:b + 1]), scale, what,
          diagonals=mask.shape[1] + labels.shape[1])


def _check_stages(case, names, cus):
    assert_stages(case["name"], stages_seen(names, P.stage_of, P.STAGES), P.predict(case, cus))


# ----------------------------------------------------------------------------- every form of tests/pruned_forms.py
def _run_loss_case(case, cus):
    N, T, U, A = P.K.case_shape(case, cus)
    S, dtype = case["S"], case["dtype"]
    x, labels, tl, ll, ranges, mask = _problem(case["name"], dtype, N, T, U, A, S)
    xv = place(x.to(DEV), case.get("off", 0), x.dtype)
    gv = place(torch.full_like(x, float("nan")).to(DEV), case.get("off", 0), x.dtype)
    (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, ranges, S, U, "one", grads=gv))
    if st == 0 and not any(P.stage_of(n) for n in names):     # (a profiler session now and then records no device event of
        print(case["name"], "no kernel of the library recorded:", names)     # the call at all: one more session, judged as the
        gv.fill_(float("nan"))                                     # first would have been)
        (st, c, g), names = profiled(lambda: call(xv, labels, tl, ll, ranges, S, U, "one", grads=gv))
    assert st == 0
    _check_stages(case, names, cus)
    assert not any(n.startswith(("rnnt::row_stats", "rnnt::grad_flat_kernel", "rnnt::grad_rows_kernel")) for n in names)
    _assert_real_lattice(c, tl, ll, ranges, S, case["name"])
    rc, rg = _reference(x, labels, tl, ll, ranges)
    _check(dtype, c, g, rc, rg, mask, labels, ranges, ll, what=case["name"])


def _run_ranges_case(case, cus):
    N, T, U, A = P.K.case_shape(case, cus)
    dtype, S = case["dtype"], case["S"]
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    tl, ll = ragged_lengths(N, T, U, rng)
    f = torch.tensor(rng.standard_normal((N, T, A)), dtype=torch.float32).to(TORCH[dtype])
    g = torch.tensor(rng.standard_normal((N, U, A)), dtype=torch.float32).to(TORCH[dtype])
    off = case.get("off", {})
    fv, gv = place(f.to(DEV), off.get("f", 0), f.dtype), place(g.to(DEV), off.get("g", 0), g.dtype)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32) if A > 1 else np.zeros((N, U - 1), np.int32)
    lab, ttl, tll = dev(labels, tl, ll)
    pl = _pl()
    out = torch.full((N, T), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(pl.workspace_bytes(T, U, N, CODE[dtype]), dtype=torch.uint8, device=DEV)

    def run():
        st = pl.lib().compute_rnnt_prune_ranges_add(fv.data_ptr(), gv.data_ptr(), lab.data_ptr(), tll.data_ptr(),
                                                    ttl.data_ptr(), A, N, S, out.data_ptr(), ws.data_ptr(), options(T, U),
                                                    CODE[dtype])
        torch.cuda.synchronize()
        return st
    st, names = profiled(run)
    if st == 0 and not any(P.stage_of(n) for n in names):     # (as _run_loss_case: one more session after an empty one)
        print(case["name"], "no kernel of the library recorded:", names)
        out.fill_(-7)
        st, names = profiled(run)
    assert st == 0
    _check_stages(case, names, cus)
    r = out.cpu().numpy()
    for b in range(N):
        Tb, L = int(tl[b]), int(ll[b])
        assert not r[b, Tb:].any()
        if L <= Tb * (S - 1):
            assert R.check_invariants(r[b], Tb, L, S) == [], (case["name"], b, r[b, :Tb])


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_pruned_form(name):
    case = P.CASES[name]
    cus = G.cus()
    if case["entry"] == "ranges":
        _run_ranges_case(case, cus)
    else:
        _run_loss_case(case, cus)


def test_every_pruned_row_reached_on_this_device():
    assert_every_row_reached(P, G.cus(), P.joint_unreachable())


# ----------------------------------------------------------------------------- call forms, equivalences, edge cases
@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
@pytest.mark.parametrize("A,U,S", [(5, 1, 1), (1, 5, 2), (64, 2, 1), (65, 64, 16), (1000, 65, 65), (5003, 9, 4)])
def test_parity_shapes(dtype, A, U, S):
    N, T = 4, 6
    x, labels, tl, ll, ranges, mask = _problem("par_%s_%d_%d_%d" % (dtype, A, U, S), dtype, N, T, U, A, S)
    st, c, g = call(x.to(DEV), labels, tl, ll, ranges, S, U, "one")
    assert st == 0
    _assert_real_lattice(c, tl, ll, ranges, S, "parity")
    rc, rg = _reference(x, labels, tl, ll, ranges)
    _check(dtype, c, g, rc, rg, mask, labels, ranges, ll, what="parity")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_call_forms_agree(dtype):
    N, T, U, A, S = 5, 7, 9, 130, 4
    x, labels, tl, ll, ranges, mask = _problem("forms_" + dtype, dtype, N, T, U, A, S)
    xd = x.to(DEV)
    st, c1, g1 = call(xd, labels, tl, ll, ranges, S, U, "one")
    assert st == 0
    scale = (0.5 + 0.25 * np.arange(N)).astype(np.float64)
    st, c2, g2 = call(xd, labels, tl, ll, ranges, S, U, "two", scale=scale)
    assert st == 0 and np.array_equal(c1, c2)
    g1s = np.where(mask[..., None], g1.astype(np.float64) * scale[:, None, None, None], 0.0)
    rc, rg = _reference(x, labels, tl, ll, ranges)
    _check(dtype, c2, g2, rc, rg, mask, labels, ranges, ll, scale=scale, what="two-phase")
    assert np.allclose(g2, g1s, rtol=1e-2 if dtype == "bf16" else 1e-6, atol=1e-6, equal_nan=True)
    xi = xd.clone()
    st, c3, g3 = call(xi, labels, tl, ll, ranges, S, U, "inplace")
    assert st == 0 and np.array_equal(c1, c3) and np.array_equal(np.nan_to_num(g3), np.nan_to_num(g1))
    st, c4, _ = call(xd, labels, tl, ll, ranges, S, U, "score")
    assert st == 0 and np.array_equal(c1, c4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st, c5, g5 = call(xd, labels, tl, ll, ranges, S, U, "one", stream=side)
    assert st == 0 and np.array_equal(c1, c5) and np.array_equal(np.nan_to_num(g5), np.nan_to_num(g1))


@pytest.mark.parametrize("dtype", ["f32", "f64", "bf16", "f16"])
def test_full_windows_equal_the_materialised_loss(dtype):
    """S = maxU, every start 0: compute_rnnt_loss_async on the same tensor."""
    from warprnnt_pytorch import _lib
    N, T, U, A = 4, 8, 6, 37
    rng = np.random.default_rng(11)
    tl, ll = ragged_lengths(N, T, U, rng)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    x = torch.tensor(rng.standard_normal((N, T, U, A)), dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    ranges = np.zeros((N, T), np.int32)
    st, c, g = call(x, labels, tl, ll, ranges, U, U, "one")
    assert st == 0
    lab, ttl, tll = dev(labels, tl, ll)
    cdt = torch.float64 if dtype == "f64" else torch.float32
    c0 = torch.empty(N, dtype=cdt, device=DEV)
    g0 = torch.empty_like(x)
    ws = torch.empty(_lib.workspace_bytes(T, U, N, True, 8 if dtype == "f64" else 4), dtype=torch.uint8, device=DEV)
    st = _lib.lib().compute_rnnt_loss_async(x.data_ptr(), g0.data_ptr(), lab.data_ptr(), tll.data_ptr(), ttl.data_ptr(), A,
                                            N, c0.data_ptr(), None, ws.data_ptr(), options(T, U), CODE[dtype])
    torch.cuda.synchronize()
    assert st == 0
    c0, g0 = c0.cpu().numpy(), g0.double().cpu().numpy()
    tol = 1e-9 if dtype == "f64" else 1e-5
    assert np.allclose(c, c0, rtol=tol, atol=tol)
    mag = np.abs(g0) + np.abs(g0).sum(-1, keepdims=True)
    O.assert_grads(g, g0, mag, TORCH[dtype], what="S = maxU")


def test_no_path_and_invalid_start():
    N, T, U, A, S = 4, 6, 8, 20, 3
    x, labels, tl, ll, ranges, mask = _problem("nopath", "f32", N, T, U, A, S)
    tl[:] = T
    ll[:] = [U - 1, 3, 2, 4]
    rng = np.random.default_rng(3)
    for b in range(N):
        ranges[b] = R.ranges_rule(rng.random((T, int(ll[b]) + 1)), T, int(ll[b]), S)
        assert R.has_path(ranges[b], T, int(ll[b]), S)
    x = torch.tensor(np.random.default_rng(4).standard_normal((N, T, S, A)), dtype=torch.float32)
    mask = R.in_lattice_mask((N, T, S), ranges, tl, ll)
    x[torch.tensor(~mask)] = float("nan")
    st, c0, g0 = call(x.to(DEV), labels, tl, ll, ranges, S, U, "one")
    assert st == 0 and np.isfinite(c0).all()
    bad = ranges.copy()
    bad[1, 3:] = 0                                          # sample 1 falls back to state 0: no path to L_b = 3
    assert not R.has_path(bad[1], T, 3, S)
    mask1 = R.in_lattice_mask((N, T, S), bad, tl, ll)
    x1 = torch.tensor(np.random.default_rng(4).standard_normal((N, T, S, A)), dtype=torch.float32)
    x1[torch.tensor(~mask1)] = float("nan")
    st, c1, g1 = call(x1.to(DEV), labels, tl, ll, bad, S, U, "one")
    assert st == 0 and np.isposinf(c1[1]) and np.isnan(g1[1][mask1[1]]).all() and not g1[1][~mask1[1]].any()
    others = np.arange(N) != 1
    assert np.array_equal(c1[others], c0[others]) and np.array_equal(g1[others], g0[others])
    invalid = ranges.copy()
    invalid[2, 1] = int(ll[2]) + 1                           # a start past L_b
    st, hc, _ = call(x.to(DEV), labels, tl, ll, invalid, S, U, "host")
    assert st == _lib_invalid()
    st, c2, g2 = call(x.to(DEV), labels, tl, ll, invalid, S, U, "one")
    assert st == 0 and np.isnan(c2[2]) and not g2[2].any() and np.array_equal(c2[others & (np.arange(N) != 2)],
                                                                               c0[others & (np.arange(N) != 2)])
    st, hc, _ = call(x.to(DEV), labels, tl, ll, ranges, S, U, "host")
    assert st == 0 and np.array_equal(hc, c0)


def _lib_invalid():
    from warprnnt_pytorch import _lib
    return _lib.RNNT_STATUS_INVALID_VALUE


def test_no_materialised_kernels_and_no_full_tensor():
    """The new streaming kernels ran, no statistics / gradient kernel of the materialised path did, and nothing of
    N * T * maxU * A elements was allocated."""
    pl = _pl()
    N, T, U, A, S = 8, 40, 21, 3000, 4
    rng = np.random.default_rng(9)
    tl = np.full(N, T, np.int32)
    ll = np.full(N, U - 1, np.int32)
    labels = torch.tensor(rng.integers(1, A, size=(N, U - 1)), dtype=torch.int32, device=DEV)
    f = torch.randn(N, T, A, device=DEV)
    g = torch.randn(N, U, A, device=DEV)
    ttl, tll = dev(tl, ll)
    ranges = pl.prune_ranges(f, g, labels, ttl, tll, S)
    logits = (f[:, :, None, :] + pl.prune_inputs(f, g, ranges, S)[1]).contiguous().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def run():
        loss = pl.rnnt_loss_pruned(logits, labels, ttl, tll, ranges)
        loss.backward()
        return loss
    _, names = profiled(run)
    peak = torch.cuda.max_memory_allocated() - base
    assert any(n.startswith("rnnt::pruned_stats_kernel") for n in names), names
    assert any(n.startswith("rnnt::pruned_grad_kernel") for n in names), names
    assert not any(n.startswith(("rnnt::row_stats", "rnnt::grad_flat_kernel", "rnnt::grad_rows_kernel")) for n in names)
    assert peak < N * T * U * A * 4, (peak, N * T * U * A * 4)


# ----------------------------------------------------------------------------- prune ranges
def _planted(N, T, U, A, rng):
    """f, g whose best alignment is clear: label u is emitted at frame ~ (u + 1) T / U (strong peaks, no near-ties)."""
    f = rng.standard_normal((N, T, A)) * 0.1
    g = rng.standard_normal((N, U, A)) * 0.1
    labels = rng.integers(1, A, size=(N, U - 1))
    for b in range(N):
        for u in range(U - 1):
            g[b, u, labels[b, u]] += 4.0
        g[b, :, 0] += 1.0
        for t in range(T):
            f[b, t, 0] += 3.0 * ((t * (U - 1)) % T < (U - 1))          # some frames prefer blank strongly
    return f, g, labels.astype(np.int32)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_prune_ranges_against_the_rule(dtype):
    pl = _pl()
    rng = np.random.default_rng(21)
    N, T, U, A, S = 6, 24, 11, 40, 4
    tl, ll = ragged_lengths(N, T, U, rng)
    tl[:] = np.maximum(tl, 4)
    # random inputs: invariants, and the occupancy the windows capture against the reference's
    f = rng.standard_normal((N, T, A))
    g = rng.standard_normal((N, U, A))
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    tf = torch.tensor(f, dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    tg = torch.tensor(g, dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    r = pl.prune_ranges(tf, tg, lab, ttl, tll, S).cpu().numpy()
    for b in range(N):
        Tb, L = int(tl[b]), int(ll[b])
        assert not r[b, Tb:].any()
        if L > Tb * (S - 1):
            assert list(r[b, :Tb]) == [min(t * (S - 1), max(0, L + 1 - S)) for t in range(Tb)]
            continue
        assert R.check_invariants(r[b], Tb, L, S) == []
        gam = R.occupancy_add(tf[b].double().cpu().numpy(), tg[b].double().cpu().numpy(), labels[b], Tb, L)
        ref = R.ranges_rule(gam, Tb, L, S)
        got_mass = sum(gam[t, r[b, t]:r[b, t] + S].sum() for t in range(Tb))
        ref_mass = sum(gam[t, ref[t]:ref[t] + S].sum() for t in range(Tb))
        assert abs(got_mass - ref_mass) <= 1e-4 * ref_mass, (b, got_mass, ref_mass)
    # planted, peaked inputs: exactly the numpy rule
    f, g, labels = _planted(N, T, U, A, rng)
    tf = torch.tensor(f, dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    tg = torch.tensor(g, dtype=torch.float32).to(TORCH[dtype]).to(DEV)
    lab = torch.tensor(labels, device=DEV)
    tl[:] = T
    ll[:] = U - 1
    ttl, tll = dev(tl, ll)
    r = pl.prune_ranges(tf, tg, lab, ttl, tll, S).cpu().numpy()
    for b in range(N):
        gam = R.occupancy_add(tf[b].double().cpu().numpy(), tg[b].double().cpu().numpy(), labels[b], T, U - 1)
        assert list(r[b]) == list(R.ranges_rule(gam, T, U - 1, S)), b
    # infeasible samples: L_b > T_b (S - 1)
    tl2 = np.array([2, 3, T, T, T, T], np.int32)
    ll2 = np.array([U - 1, U - 1, 2, 0, 5, U - 1], np.int32)
    ttl, tll = dev(tl2, ll2)
    r = pl.prune_ranges(tf, tg, lab, ttl, tll, S).cpu().numpy()
    for b in (0, 1):
        Tb, L = int(tl2[b]), int(ll2[b])
        assert list(r[b, :Tb]) == [min(t * (S - 1), L + 1 - S) for t in range(Tb)] and not r[b, Tb:].any()


# ----------------------------------------------------------------------------- end to end
def _peaked(N, T, U, A, rng):
    """f, g of one dominant alignment: blank everywhere (f[t, blank] = 10) except at frame tau_u, where f holds +20 on label u
    (distinct labels per sample); nearly all the path mass lies on that alignment."""
    f = rng.standard_normal((N, T, A)) * 0.01
    g = rng.standard_normal((N, U, A)) * 0.01
    labels = np.zeros((N, U - 1), np.int32)
    f[:, :, 0] += 10.0
    for b in range(N):
        labels[b] = rng.permutation(np.arange(1, A))[:U - 1]
        for u in range(U - 1):
            tau = (u + 1) * T // U
            f[b, tau, labels[b, u]] += 20.0
    return f, g, labels


def test_recipe_against_the_additive_joint():
    from warprnnt_pytorch.add_network import RNNTLossAdd
    pl = _pl()
    rng = np.random.default_rng(5)
    N, T, U, A = 4, 30, 9, 50
    f, g, labels = _peaked(N, T, U, A, rng)
    tl = np.full(N, T, np.int32)
    ll = np.full(N, U - 1, np.int32)
    tf, tg = torch.tensor(f, dtype=torch.float32, device=DEV), torch.tensor(g, dtype=torch.float32, device=DEV)
    lab, ttl, tll = dev(labels, tl, ll)
    simple = RNNTLossAdd(reduction="none")(tf, tg, lab, ttl, tll)
    for S, tol in ((U, 1e-5), (4, 1e-3)):
        r = pl.prune_ranges(tf, tg, lab, ttl, tll, S)
        am, lm = pl.prune_inputs(tf, tg, r, S)
        loss = pl.rnnt_loss_pruned((am + lm).contiguous(), lab, ttl, tll, r, reduction="none")
        assert (loss >= simple - 1e-4 * simple.abs()).all()
        assert torch.allclose(loss, simple, rtol=tol, atol=tol), (S, loss, simple)
    rnd = torch.randn(N, T, A, device=DEV), torch.randn(N, U, A, device=DEV)
    base = RNNTLossAdd(reduction="none")(rnd[0], rnd[1], lab, ttl, tll)
    r = pl.prune_ranges(rnd[0], rnd[1], lab, ttl, tll, 3)
    am, lm = pl.prune_inputs(rnd[0], rnd[1], r, 3)
    loss = pl.rnnt_loss_pruned((am + lm).contiguous(), lab, ttl, tll, r, reduction="none")
    assert (loss >= base - 1e-4 * base.abs()).all()


def test_backprop_through_a_joiner():
    """RNNTLossPruned through a small fp64 Linear + tanh + Linear joiner: the input gradients of pruned_ref."""
    pl = _pl()
    torch.manual_seed(0)
    rng = np.random.default_rng(8)
    N, T, U, D, H, A, S = 3, 7, 6, 5, 8, 11, 3
    tl = np.array([T, 5, 3], np.int32)
    ll = np.array([U - 1, 2, 4], np.int32)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    ranges = np.zeros((N, T), np.int32)
    for b in range(N):
        ranges[b, :tl[b]] = R.ranges_rule(rng.random((tl[b], ll[b] + 1)), int(tl[b]), int(ll[b]), S)
    am0 = torch.randn(N, T, D, dtype=torch.float64)
    lm0 = torch.randn(N, U, D, dtype=torch.float64)
    j1, j2 = torch.nn.Linear(D, H).double(), torch.nn.Linear(H, A).double()

    def joiner(a, l):
        return j2(torch.tanh(j1(a + l)))
    am, lm = am0.to(DEV).requires_grad_(True), lm0.to(DEV).requires_grad_(True)
    j1.to(DEV), j2.to(DEV)
    lab, ttl, tll, tr = dev(labels, tl, ll, ranges)
    a_p, l_p = pl.prune_inputs(am, lm, tr, S)
    loss = pl.RNNTLossPruned(reduction="sum")(joiner(a_p, l_p).contiguous(), lab, ttl, tll, tr)
    loss.backward()
    j1.cpu(), j2.cpu()
    am_c, lm_c = am0.clone().requires_grad_(True), lm0.clone().requires_grad_(True)
    a_p, l_p = pl.prune_inputs(am_c, lm_c, torch.tensor(ranges), S)
    z = joiner(a_p, l_p)
    costs = [R._sample_pruned(z[b, :tl[b]], ranges[b], labels[b], int(tl[b]), int(ll[b]), 0) for b in range(N)]
    sum(costs).backward()
    assert abs(loss.item() - sum(c.item() for c in costs)) < 1e-9 * abs(loss.item())
    assert torch.allclose(am.grad.cpu(), am_c.grad, rtol=1e-8, atol=1e-10)
    assert torch.allclose(lm.grad.cpu(), lm_c.grad, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_autograd_reductions_and_grad_output(dtype):
    """RNNTLossPruned's values and gradients under 'sum', 'mean' (with grad_output 3) and 'none' (a grad_output vector): the
    1/N and grad_output factors folded into the gradient kernel's per-sample scale."""
    pl = _pl()
    rng = np.random.default_rng(31)
    N, T, U, A, S = 4, 6, 5, 9, 3
    tl = np.full(N, T, np.int32)
    tl[1] = 4
    ll = np.array([U - 1, 2, 0, 3], np.int32)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    ranges = np.zeros((N, T), np.int32)
    for b in range(N):
        ranges[b, :tl[b]] = R.ranges_rule(rng.random((tl[b], ll[b] + 1)), int(tl[b]), int(ll[b]), S)
    mask = R.in_lattice_mask((N, T, S), ranges, tl, ll)
    x0 = torch.tensor(rng.standard_normal((N, T, S, A)), dtype=TORCH[dtype])
    x0[torch.tensor(~mask)] = float("nan")
    lab, ttl, tll, tr = dev(labels, tl, ll, ranges)
    w = np.array([0.5, 2.0, -1.0, 1.5])
    ref_c, ref_g = _reference(x0, labels, tl, ll, ranges)
    _, ref_gw = _reference(x0, labels, tl, ll, ranges, weights=w)
    tol = dict(rtol=1e-9, atol=1e-12) if dtype == "f64" else dict(rtol=1e-4, atol=1e-6)

    def run(reduction, grad):
        x = x0.to(DEV).requires_grad_(True)
        loss = pl.rnnt_loss_pruned(x, lab, ttl, tll, tr, reduction=reduction)
        loss.backward(grad)
        return loss.detach().double().cpu().numpy(), x.grad.double().cpu().numpy()
    c_sum, g_sum = run("sum", torch.ones(1, dtype=x0.dtype, device=DEV))
    c_mean, g_mean = run("mean", torch.full((1,), 3.0, dtype=x0.dtype, device=DEV))
    c_none, g_none = run("none", torch.tensor(w, dtype=x0.dtype, device=DEV))
    assert np.allclose(c_none, ref_c, **tol) and np.allclose(c_sum, ref_c.sum(), **tol)
    assert np.allclose(c_mean, ref_c.sum() / N, **tol)
    for g in (g_sum, g_mean, g_none):
        assert not g[~mask].any()
    assert np.allclose(g_sum[mask], ref_g[mask], **tol)
    assert np.allclose(g_mean[mask], 3.0 / N * ref_g[mask], **tol)
    assert np.allclose(g_mean[mask], 3.0 / N * g_sum[mask], **tol)
    assert np.allclose(g_none[mask], ref_gw[mask], **tol)


def test_autograd_without_labels():
    """maxU = 1: an empty (N, 0) label tensor through the PyTorch wrapper, S = 1, every start 0."""
    pl = _pl()
    rng = np.random.default_rng(32)
    N, T, A = 3, 5, 7
    tl = np.array([T, 2, 4], np.int32)
    ll = np.zeros(N, np.int32)
    labels = np.zeros((N, 0), np.int32)
    ranges = np.zeros((N, T), np.int32)
    x0 = torch.tensor(rng.standard_normal((N, T, 1, A)), dtype=torch.float32)
    mask = R.in_lattice_mask((N, T, 1), ranges, tl, ll)
    x0[torch.tensor(~mask)] = float("nan")
    ref_c, ref_g = _reference(x0, labels, tl, ll, ranges)
    x = x0.to(DEV).requires_grad_(True)
    ttl, tll, tr = dev(tl, ll, ranges)
    lab = torch.zeros((N, 0), dtype=torch.int32, device=DEV)
    loss = pl.rnnt_loss_pruned(x, lab, ttl, tll, tr, reduction="none")
    loss.sum().backward()
    g = x.grad.double().cpu().numpy()
    assert np.allclose(loss.detach().cpu().numpy(), ref_c, rtol=1e-5)
    assert not g[~mask].any() and np.allclose(g[mask], ref_g[mask], rtol=1e-4, atol=1e-6)
