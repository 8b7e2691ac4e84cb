"""No GPU: tests/side_limits.py against the sources (every sliced, whole-N and capped launch of csrc/rnnt_*_impl.h, name for
name, through tests/launch_scan.py), against the built code objects (every sliced or capped instantiation has a row of its
object), the arithmetic of every row, and the comparison itself with planted faults: a second slice that repeats the first,
one left unwritten, one scaled with the first slice's scales -- each must be refused by fold() + the module's checker, and the
reference must pass."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import hat_ref as R
from tests import inventory as I
from tests import launch_scan as L
from tests import side_limits as SL
from tests.forms_common import STORES
from tests.side_check import check, in_lattice_mask


# ----------------------------------------------------------------------------- the table against the sources
def test_the_scanner_reads_every_launch():
    """Exactly one read statement per hipLaunchKernelGGL statement of the sources (comments aside), each with a kernel name
    that the library's kernel header defines."""
    for lib in L.SIDE:
        text = re.sub(r"//[^\n]*", "", open(os.path.join(L.CSRC, "rnnt_%s_impl.h" % lib)).read())
        got = L.launches(lib)
        assert len({l["stmt"] for l in got}) == len(re.findall(r"hipLaunchKernelGGL\(", text)) > 0, lib
        for l in got:
            assert re.fullmatch(r"[a-z0-9_]+_kernel", l["kernel"]), (lib, l)


def test_grid_samples_is_the_sources():
    text = open(os.path.join(L.CSRC, "rnnt_kernels.h")).read()
    assert int(re.search(r"constexpr int kGridSamples = (\d+);", text).group(1)) == SL.GRID_SAMPLES
    host = open(os.path.join(L.CSRC, "rnnt_side_host.h")).read()
    assert "blocks < 65536 ? (blocks ? blocks : 1) : 65536" in host and SL.ELEM_BLOCKS == 65536
    assert "(E + 255) / 256" in host and SL.ELEM_THREADS == 256
    for lib, const, grid in (("joiner", "kJnMaxGrid", "jn_row_grid"), ("logprobs", "kLpMaxGrid", "lp_grid")):
        srcs = "".join(open(os.path.join(L.CSRC, "rnnt_%s_%s.h" % (lib, f))).read() for f in ("impl", "kernels"))
        m = re.search(r"constexpr long long %s = 1 << (\d+);" % const, srcs)
        assert m and 1 << int(m.group(1)) == SL.TRIPS[grid]["cap"], (lib, const)


@pytest.mark.parametrize("lib", L.SIDE)
def test_sliced_launches_are_the_sources(lib):
    """A sliced or whole-N launch that the table does not name, or names but the sources do not have, fails here."""
    got = L.by_class(lib)
    assert got.get("sliced", set()) == SL.SLICED[lib]["kernels"], lib
    assert got.get("whole_n", set()) == set(SL.SLICED[lib]["whole_n"]), lib


def test_capped_launches_are_the_sources():
    for grid, klass in (("elem_grid", "elem"), ("jn_row_grid", "jn_row"), ("lp_grid", "lp")):
        want = {}
        for lib in L.SIDE:
            ks = L.by_class(lib).get(klass)
            if ks:
                want[lib] = ks
        users = SL.TRIPS[grid]["users"]
        assert {lib: ({k} if isinstance(k, str) else set(k)) for lib, k in users.items()} == want, grid


def test_every_library_with_a_sliced_launch_has_rows():
    with_rows = {r["lib"] for r in SL.ROWS.values()}
    for lib in L.SIDE:
        if SL.SLICED[lib]["kernels"]:
            assert lib in with_rows, lib
    assert with_rows == set(SL.LIBS + SL.WHOLE_N_LIBS)
    for lib in SL.WHOLE_N_LIBS:
        assert SL.SLICED[lib]["whole_n"] and not SL.SLICED[lib]["kernels"]


# ----------------------------------------------------------------------------- the built code objects
def _twin(kernel):
    """F16 shares BF16's code object and launch code: the table's rows take one 16-bit storage type."""
    return kernel.replace("rnnt::F16", "rnnt::BF16")


@pytest.mark.parametrize("lib", SL.LIBS)
def test_every_sliced_instantiation_has_a_row(lib):
    """Every instantiation of a sliced kernel in the library's code objects (the forms table's expected_inventory(), which the
    library's own CPU test holds to the objects; here the objects again) is launched by a row of that object."""
    F = SL.forms_of(lib)
    built = I.side_inventory(I.need_lib("libwarprnnt_%s.so" % lib))
    want = F.expected_inventory()
    cov = SL.covered(lib)
    for obj, ks in want.items():
        assert built[obj] == ks, (lib, obj)
        for k in ks:
            base = k.split("<")[0].split("::")[-1]
            if base in SL.ALL_SLICED and (lib, base) not in SL.REFUSED:
                assert _twin(k) in cov.get(obj, set()), (lib, obj, k)


def test_every_capped_instantiation_has_a_row_or_a_reason():
    for lib, base in SL.TRIPS["elem_grid"]["users"].items():
        F = SL.forms_of(lib)
        I.need_lib("libwarprnnt_%s.so" % lib)
        reached = {(STORES[r["dtype"]][0], SL.trip_kernel(r)) for r in SL.TRIP_ROWS.values() if r["lib"] == lib}
        for obj, ks in F.expected_inventory().items():
            for k in ks:
                if k.split("<")[0].split("::")[-1] == base:
                    assert (obj, _twin(k)) in reached, (lib, obj, k)
    # jn_row_grid: every instantiation of its kernels has a row of its object that takes it into a second trip, or a reason
    F = SL.forms_of("joiner")
    I.need_lib("libwarprnnt_joiner.so")
    reached = {(STORES[r["dtype"]][0], k) for r in SL.JN_ROWS.values() for k in SL.jn_kernels(r)}
    for obj, ks in F.expected_inventory().items():
        for k in ks:
            base = k.split("<")[0].split("::")[-1]
            if base in SL.TRIPS["jn_row_grid"]["users"]["joiner"]:
                assert (obj, _twin(k)) in reached or ("joiner", base) in SL.UNREACHABLE, (obj, k)
    assert not SL.NOT_BUILT
    # lp_grid: every instantiation of its two kernels has a row of its object (BF16 for F16)
    F = SL.forms_of("logprobs")
    I.need_lib("libwarprnnt_logprobs.so")
    reached = {(STORES[r["dtype"]][0], k) for r in SL.LP_ROWS.values() for ks in F.predict(r).values() for k in ks}
    for obj, ks in F.expected_inventory().items():
        for k in ks:
            if k.split("<")[0].split("::")[-1] in SL.TRIPS["lp_grid"]["users"]["logprobs"]:
                assert (obj, _twin(k)) in reached, (obj, k)


@pytest.mark.parametrize("name", sorted(SL.LP_ROWS))
def test_logprobs_trip_row_arithmetic(name):
    row = SL.LP_ROWS[name]
    for k, (work, per) in SL.lp_work(row).items():
        assert work > SL.LP_CAP * per and SL.lp_trips(row)[k] >= 2, (name, k, work, per)
    assert SL.lp_bytes(row) <= SL.BUDGET
    e = STORES[row["dtype"]][3]
    assert (SL.lp_px(row) == 1) == ((row["C"] * e) % 16 == 0 and row["C"] * e == 16)


@pytest.mark.parametrize("name", sorted(SL.JN_ROWS))
def test_joiner_trip_row_arithmetic(name):
    row = SL.JN_ROWS[name]
    trips, work = SL.jn_trips(row), SL.jn_work(row)
    want = ("joiner_fwd_kernel", "joiner_df_kernel" if row["heavy"] == "f" else "joiner_dg_kernel")
    for k in want:
        assert work[k][0] > SL.JN_CAP * work[k][1] and trips[k] == 2, (name, k, work[k])
    assert {k.split("<")[0].split("::")[-1] for k in SL.jn_kernels(row)} == set(want)
    assert SL.jn_bytes(row) <= SL.BUDGET and row["N"] > SL.GRID_SAMPLES
    e = STORES[row["dtype"]][3]
    assert SL.jn_px(row) == 1 and row["H"] * e in (e, 16)
    stages = SL.forms_of("joiner").predict({k: v for k, v in row.items() if k not in ("lib", "grid", "heavy")})
    assert "df" in stages and "dg" in stages and "bwd" not in stages and "sum" not in stages


# ----------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("name", sorted(SL.ROWS))
def test_row_arithmetic(name):
    row = SL.ROWS[name]
    assert row["N"] > SL.GRID_SAMPLES and SL.slices(row) == 2
    assert row["N"] % SL.GRID_SAMPLES >= 1 and row["N"] >= SL.PERIOD
    assert SL.kernels(row), name                                       # the row names a sliced kernel at least
    assert row["dtype"] in SL.DTYPES
    e = SL.elements(row)
    assert e * 8 <= SL.HOST_BUDGET, (name, e)
    assert 4 * e * 8 <= SL.BUDGET
    # the block-phase rule: the second slice starts at another block position and another scale
    assert SL.GRID_SAMPLES % SL.K == 1 and SL.GRID_SAMPLES % SL.P == 3
    c = SL.block_case(row)
    assert c["N"] == SL.K and c["name"] == name


def test_second_slice_holds_every_block_position():
    assert SL.NS[0] - SL.GRID_SAMPLES == 1 and SL.NS[1] - SL.GRID_SAMPLES >= SL.K
    for lib in SL.LIBS + SL.WHOLE_N_LIBS:
        for d in SL.DTYPES:
            ns = {r["N"] for r in SL.ROWS.values() if r["lib"] == lib and r["dtype"] == d}
            assert ns == set(SL.NS), (lib, d, ns)


@pytest.mark.parametrize("name", sorted(SL.TRIP_ROWS))
def test_trip_row_arithmetic(name):
    row = SL.TRIP_ROWS[name]
    e = SL.trip_elements(row)
    assert e > SL.ELEM_BLOCKS * SL.ELEM_THREADS and SL.trips(row) == 2
    assert e * 8 * 4 <= SL.HOST_BUDGET * 2 and e * 8 * 4 <= SL.BUDGET
    b, r, col = SL.trip_boundary(row)
    assert b == row["N"] - 1 and row["lengths"][0][b] == row["T"] and row["lengths"][1][b] == row["U"] - 1, (b, r, col)
    assert row["off"] == STORES[row["dtype"]][3] and row["off"] % 16 != 0
    assert SL.trip_kernel(row).split("<")[0].endswith(SL.TRIPS["elem_grid"]["users"][row["lib"]])


def test_joiner_rows_take_the_two_pass_backward():
    """Past 65535 samples jn_plan leaves the single pass (N on grid.y): the rows predict joiner_df_kernel and joiner_dg_kernel,
    the same shape at N = 65535 joiner_bwd_kernel; the pruned layout's rows launch joiner_prep_kernel with N on grid.x."""
    F = SL.forms_of("joiner")
    for row in SL.ROWS.values():
        if row["lib"] != "joiner":
            continue
        stages = F.predict(SL.full_case(row))
        assert "df" in stages and "dg" in stages and "bwd" not in stages, row["name"]
        assert "bwd" in F.predict(dict(SL.full_case(row), N=SL.GRID_SAMPLES))
        assert ("prep" in stages) == (row["layout"] == 2)


def test_unreachable_arithmetic():
    """joiner_dg_sum_kernel: the largest E the single-pass route with shares allows stays under one trip."""
    best = 0
    for N in (1, 2, 7, 15, 1023):
        for H in range(1, 70000, 63):
            if N * ((H + 63) // 64) < 1024:
                best = max(best, N * 256 * H)
    assert best < SL.TRIPS["jn_row_grid"]["cap"] * 256


# ----------------------------------------------------------------------------- planted faults
N_BIG, T, U, A, BLANK = SL.NS[1], 3, 3, 4, 1
_RNG = np.random.default_rng(7)
TL, LL = np.array([3, 1, 2, 2, 3, 1, 2], np.int32), np.array([2, 1, 0, 2, 1, 0, 1], np.int32)
LABELS = _RNG.integers(2, A, size=(SL.K, U - 1)).astype(np.int32)
MASK = in_lattice_mask((SL.K, T, U), TL, LL)
REF_C, REF_G = R.hat_autograd(_RNG.standard_normal((SL.K, T, U, A)) * 2.0, LABELS, TL, LL, BLANK)


def _mag(labels, ll):
    def mag_of(ref, b):
        mag = np.abs(ref).copy()
        rs = np.abs(ref).sum(-1)
        mag[..., BLANK] = np.maximum(mag[..., BLANK], rs)
        for u in range(int(ll[b])):
            mag[0, :, u, labels[b, u]] = np.maximum(mag[0, :, u, labels[b, u]], rs[0, :, u])
        return mag
    return mag_of


def _judge(costs, grads, scaled, dtype="f32"):
    """What tests/test_gpu_side_limits.py does with a library's outputs: fold, then the checker against the repeated block."""
    rc, rg, mask = SL.tile(REF_C, SL.PERIOD), SL.tile(REF_G, SL.PERIOD), SL.tile(MASK, SL.PERIOD)
    labels, ll = SL.tile(LABELS, SL.PERIOD), SL.tile(LL, SL.PERIOD)
    SL.check_folded(dict(costs=costs, grads=grads),
                    lambda o, scale: check(dtype, o["costs"], o["grads"], rc, rg, mask, _mag(labels, ll), scale, "planted",
                                           infinite_ok=False), scaled)


def _faithful(n, scaled):
    c, g = SL.tile(REF_C, n), SL.tile(REF_G, n)
    if scaled:
        g = g * SL.scale_of(n)[:, None, None, None]
    return c, g


@pytest.mark.parametrize("n", SL.NS)
@pytest.mark.parametrize("scaled", [False, True])
def test_the_repeated_reference_passes(n, scaled):
    assert np.isfinite(REF_C).all() and REF_G[MASK].any()
    _judge(*_faithful(n, scaled), scaled)


@pytest.mark.parametrize("n", SL.NS)
@pytest.mark.parametrize("scaled", [False, True])
def test_a_second_slice_that_repeats_the_first_is_refused(n, scaled):
    """(a) a kernel without b0: samples b >= 65535 are computed from the data of sample b - 65535."""
    c, g = _faithful(n, scaled)
    c[SL.GRID_SAMPLES:] = c[:n - SL.GRID_SAMPLES]
    with pytest.raises(AssertionError):
        _judge(c, _faithful(n, scaled)[1], scaled)
    g[SL.GRID_SAMPLES:] = g[:n - SL.GRID_SAMPLES]
    with pytest.raises(AssertionError):
        _judge(_faithful(n, scaled)[0], g, scaled)


@pytest.mark.parametrize("n", SL.NS)
def test_an_unwritten_second_slice_is_refused(n):
    """(b) samples b >= 65535 keep the NaN they started with -- in the costs, in the gradients, in one sample of them."""
    c, g = _faithful(n, False)
    c[SL.GRID_SAMPLES:] = np.nan
    with pytest.raises(AssertionError):
        _judge(c, g, False)
    c, g = _faithful(n, False)
    g[SL.GRID_SAMPLES:] = np.nan
    with pytest.raises(AssertionError):
        _judge(c, g, False)
    c, g = _faithful(n, False)
    g[n - 1] = np.nan
    with pytest.raises(AssertionError):
        _judge(c, g, False)


@pytest.mark.parametrize("n", SL.NS)
def test_the_first_slices_scale_in_the_second_is_refused(n):
    """(c) grad_scale[b - b0] in the place of grad_scale[b]."""
    c, g = SL.tile(REF_C, n), SL.tile(REF_G, n)
    s = SL.scale_of(n).copy()
    s[SL.GRID_SAMPLES:] = s[:n - SL.GRID_SAMPLES]
    assert (s[SL.GRID_SAMPLES:] != SL.scale_of(n)[SL.GRID_SAMPLES:]).all()
    with pytest.raises(AssertionError):
        _judge(c, g * s[:, None, None, None], True)


def test_one_element_of_one_sample_past_its_bound_is_refused():
    """Every sample is compared: one element of one sample deep in the second slice, three bounds off, fails; half a bound
    passes."""
    n = SL.NS[1]
    c, g = _faithful(n, False)
    b = n - 3
    k = b % SL.K
    t, u = 0, 0
    assert MASK[k, t, u]
    bound = O.grad_bound(REF_G[k, t, u, BLANK], _mag(LABELS, LL)(REF_G[k:k + 1], k)[0, t, u, BLANK], "float32")
    g[b, t, u, BLANK] += 0.5 * bound
    _judge(c, g, False)
    g[b, t, u, BLANK] += 2.5 * bound
    with pytest.raises(AssertionError):
        _judge(c, g, False)
    g = _faithful(n, False)[1]
    g[b, t, u, BLANK] -= 3.0 * bound
    with pytest.raises(AssertionError):
        _judge(c, g, False)
    g = _faithful(n, False)[1]
    pad = tuple(np.argwhere(~MASK[k])[0])
    g[(b,) + pad + (0,)] = 1e-30
    with pytest.raises(AssertionError, match="padding"):
        _judge(c, g, False)
