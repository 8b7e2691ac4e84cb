"""The side libraries past their grid limits: one row per case that takes a launch of csrc/rnnt_*_impl.h past a limit of its
grid, in the style of tests/large_forms.py.  tests/test_side_limits_table.py checks the table without a GPU (against the
sources, the built code objects, the arithmetic of every row, planted faults in the comparison);
tests/test_gpu_side_limits.py runs every row on the GPU.

SLICED: the launches with the samples on a grid dimension in slices of kGridSamples = 65535 (`for (int b0 ...`, the kernel
computes b = b0 + blockIdx) and the launches with N itself on a grid dimension, per library.  ROWS: the cases with N > 65535.
A row is a batch of N samples made by repeating a ragged base block of K = 7 samples -- the batch of K samples the library's
own generators give for the row's name: sample 0 full size, sample 1 with T_b = 1, sample 2 with L_b = 0, the rest from the
name (for mi and bestpath: the seven rectangle patterns of their tables).  kGridSamples mod K = 1: sample 65535 + i sits at
another block position than sample i, so a kernel that drops b0 reads other data, not an identical copy.  The two-phase form
takes a per-sample scale of period P = 4 (coprime to K, no value 1, kGridSamples mod P = 3: a scale read at b - b0 is
another one).  The fp64 reference of the module is computed once, for the block, and repeated; every sample of the batch is
compared: fold() reduces the batch to the element-wise largest and smallest value of every class of samples b mod K P (NaN
kept, its pattern identical over a class), and the module's own checker at its own bounds judges both -- what holds for the
largest and the smallest holds for every sample between them.

TRIPS: the capped grids with grid-stride loops.  elem_grid (csrc/rnnt_side_host.h): at most 65536 blocks of 256 threads,
one element per thread and trip; TRIP_ROWS has a row per user and storage type with E just over 2^24 elements, the logits
(and kd's teacher) one element past a 16-byte boundary.  The flat packet kernels (Tune::gmax = 4194304 blocks x 512 packets
x 16 bytes = 34.4 GB per tensor before a second round) are out of scope.  The joiner's row grid (jn_row_grid, kJnMaxGrid =
2^20 blocks) and the logprobs grid (lp_grid, kLpMaxGrid = 2^20 blocks) are listed in TRIPS with their arithmetic; LP_ROWS takes
logprobs_edges_kernel and both forms of logprobs_grad_kernel into their second trip (2^28 + 8 rows of 2 to 8 columns), the
JN_ROWS does the same for joiner_fwd_kernel, joiner_df_kernel
and joiner_dg_kernel (2^28 + 2^16 rows of one packet or one element); joiner_dg_sum_kernel is UNREACHABLE."""
import math
import zlib

import numpy as np

from tests.forms_common import STORES

K = 7                                  # samples of the base block
GRID_SAMPLES = 65535                   # kGridSamples (csrc/rnnt_kernels.h)
NS = (65536, 65548)                    # a second slice of one sample; a second slice holding every block position
SCALE = (0.5, 1.5, 0.75, 2.0)          # the per-sample scale of the two-phase form, by b mod P
P = len(SCALE)
PERIOD = K * P                         # samples b, b' with b = b' mod PERIOD hold the same data and the same scale
DTYPES = ("f32", "f64", "bf16")        # one row per code object: F16 shares BF16's object and its launch code
BUDGET = 48 * 10 ** 9                  # tests/large_forms.py: peak device bytes of one row
HOST_BUDGET = 3 * 10 ** 9              # bytes of a row's largest output as float64 on the host: rows take seconds

assert GRID_SAMPLES % K != 0, "sample 65535 + i must sit at another block position than sample i"
assert math.gcd(K, P) == 1 and GRID_SAMPLES % P != 0 and 1.0 not in SCALE and len(set(SCALE)) == P
assert all(n > GRID_SAMPLES for n in NS) and NS[1] - GRID_SAMPLES >= K and NS[1] % PERIOD == 0


def scale_of(n):
    return np.asarray(SCALE, np.float64)[np.arange(n) % P]


def tile(a, n):
    """An array or tensor whose first axis is the base block (or any period of it), repeated along it to n samples."""
    reps = -(-n // a.shape[0])
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n])
    return a.repeat((reps,) + (1,) * (a.dim() - 1))[:n].contiguous()


def fold(got, what=""):
    """(hi, lo) of shape (PERIOD, ...): the element-wise largest and smallest value over the samples of every class b mod
    PERIOD of `got` (N, ...).  A NaN in any sample of a class is kept in both, and the NaN pattern must be the same in every
    sample of a class."""
    got = np.asarray(got)
    n = got.shape[0]
    full, rest = divmod(n, PERIOD)
    assert full >= 1, (what, n)
    body = got[:full * PERIOD].reshape((full, PERIOD) + got.shape[1:])
    hi, lo = body.max(0), body.min(0)
    tail = got[full * PERIOD:]
    if got.dtype.kind == "f":
        nans = np.isnan(body).sum(0)
        assert ((nans == 0) | (nans == full)).all(), (what, "NaN in some samples of a class and not in others",
                                                      np.argwhere((nans != 0) & (nans != full))[:4])
        assert np.array_equal(np.isnan(tail), nans[:rest] == full), (what, "NaN pattern of the last samples")
    hi[:rest], lo[:rest] = np.maximum(hi[:rest], tail), np.minimum(lo[:rest], tail)
    return hi, lo


def check_folded(outs, check, scaled):
    """check({name: (PERIOD, ...) array}, scale or None) on the largest and on the smallest values of `outs` ({name: (N, ...)
    array or None}).  scaled: the call took scale_of(N)."""
    folds = {k: fold(v, k) for k, v in outs.items() if v is not None}
    for side in (0, 1):
        check({k: f[side] for k, f in folds.items()}, scale_of(PERIOD) if scaled else None)


# ----------------------------------------------------------------------------- the sliced launches, per library
_N_ON_X = "N on grid.x: up to 2^31 - 1 blocks, no limit below the int N itself"
SLICED = {
    "tdt": dict(kernels={"tdt_stats_kernel", "tdt_lattice_kernel", "tdt_coef_kernel"}, whole_n={}),
    "mblank": dict(kernels={"mblank_stats_kernel", "mblank_lattice_kernel", "mblank_coef_kernel"}, whole_n={}),
    "mono": dict(kernels={"mono_stats_kernel", "mono_lattice_wave_kernel", "mono_lattice_block_kernel", "mono_coef_kernel"},
                 whole_n={}),
    "ar": dict(kernels={"ar_bounds_kernel", "ar_stats_kernel", "ar_lattice_wave_kernel", "ar_lattice_block_kernel",
                        "ar_coef_kernel"}, whole_n={}),
    "delay": dict(kernels={"delay_stats_kernel", "ar_lattice_wave_kernel", "ar_lattice_block_kernel", "delay_emit_kernel",
                           "delay_coef_kernel"}, whole_n={}),
    "pstream": dict(kernels={"pstream_prep_kernel", "pstream_stats_kernel", "ar_lattice_wave_kernel", "ar_lattice_block_kernel",
                             "mono_lattice_wave_kernel", "mono_lattice_block_kernel", "pstream_coef_kernel"}, whole_n={}),
    "pruned": dict(kernels={"pruned_prep_kernel", "pruned_stats_kernel", "pruned_window_kernel"}, whole_n={}),
    "hat": dict(kernels={"hat_stats_kernel"}, whole_n={}),
    "kd": dict(kernels={"kd_stats_kernel"}, whole_n={"kd_cost_kernel": _N_ON_X}),
    "mi": dict(kernels={"mi_pack_kernel", "ar_lattice_wave_kernel", "ar_lattice_block_kernel", "mono_lattice_wave_kernel",
                        "mono_lattice_block_kernel", "mi_unpack_kernel"}, whole_n={}),
    "bestpath": dict(kernels={"bestpath_edges_kernel"}, whole_n={"bestpath_sweep_kernel": _N_ON_X}),
    "tdt_align": dict(kernels={"tdt_align_lattice_kernel"}, whole_n={}),
    "joiner": dict(kernels=set(), whole_n={
        "joiner_prep_kernel": _N_ON_X,
        "joiner_bwd_kernel": "N on grid.y behind jn_plan's rule single = ... && N <= 65535: a larger batch takes joiner_df_kernel "
                             "and joiner_dg_kernel"}),
    "logprobs": dict(kernels=set(), whole_n={}),
}
# a library's driver also runs the sliced launchers of the headers it includes (tdt_align: launch_tdt_stats; pstream, delay:
# the lattices of ar / mono): a row names every sliced kernel its forms table predicts, whichever header launches it
ALL_SLICED = set().union(*(s["kernels"] for s in SLICED.values()))


def forms_of(lib):
    import importlib
    return importlib.import_module("tests.%s_forms" % lib)


# ----------------------------------------------------------------------------- the rows
def _widths(d, wide=2048):
    """A of the 16- and of the 64-lane statistics form: one element past the 4-lane and the 16-lane row sizes."""
    e = STORES[d][3]
    return 256 // e + 1, wide // e + 1


def _stats_rows(d, wide=2048, kw=lambda a: {}):
    """The wider statistics forms on the smallest lattice that still has a label: 2 x 2 rows (16 lanes), 1 x 2 rows (64)."""
    a16, a64 = _widths(d, wide)
    return [("g16", (NS[1],), dict(T=2, U=2, A=a16, **kw(a16))), ("g64", (NS[0],), dict(T=1, U=2, A=a64, **kw(a64)))]


def _variants(lib, d, i):
    """[(tag, Ns, fields)] of one library and storage type (i: its index, to alternate types and modes)."""
    if lib == "hat":
        return [("small", NS, dict(T=3, U=3, A=4, blank=1))] + _stats_rows(d, 4096, kw=lambda a: dict(blank=a - 1))
    if lib == "tdt":
        return [("small", NS, dict(T=3, U=3, A=4, durations=(0, 1, 2)))] + _stats_rows(d, kw=lambda a: dict(durations=(0, 1)))
    if lib == "tdt_align":
        return [("small", NS, dict(T=3, U=3, A=4, durations=(0, 1, 2))),
                ("u65", NS[1:], dict(T=2, U=65, A=3, durations=(0, 1)))] + _stats_rows(d, kw=lambda a: dict(durations=(0, 1)))
    if lib == "mblank":
        return [("small", NS, dict(T=3, U=3, A=5, blank=4, columns=(3,), durations=(2,)))] + \
            _stats_rows(d, kw=lambda a: dict(blank=0, columns=(a - 1,), durations=(2,)))
    if lib == "kd":
        return [("small_m%d" % m, (NS[(i + m) % 2],), dict(T=3, U=3, A=4, blank=1, mode=m)) for m in (0, 1)] + \
            [(t + "_m%d" % m, ns, dict(f, mode=m)) for m in (0, 1) for t, ns, f in _stats_rows(d, kw=lambda a: dict(blank=a // 2))]
    if lib in ("ar", "mono"):
        return [("small", NS, dict(T=3, U=3, A=4, blank=3)), ("u65", NS[1:], dict(T=2, U=65, A=3, blank=2))] + \
            _stats_rows(d, kw=lambda a: dict(blank=0))
    if lib == "delay":                 # U = 66: the block lattice and the emission kernel's form past 64 label columns
        return [("small", NS, dict(T=3, U=3, A=4, blank=3)), ("u66", NS[1:], dict(T=2, U=66, A=3, blank=2))] + \
            _stats_rows(d, kw=lambda a: dict(blank=0))
    if lib == "pstream":
        return [("small_t%d" % t, (NS[(i + t) % 2],), dict(T=3, U=3, S=2, A=4, blank=3, type=t)) for t in (0, 1)] + \
            [("u65_t%d" % t, NS[1:], dict(T=2, U=65, S=3, A=3, blank=2, type=t)) for t in (0, 1)] + \
            [(t, ns, dict(f, S=2, type=i % 2)) for t, ns, f in _stats_rows(d, kw=lambda a: dict(blank=0))]
    if lib == "pruned":
        return [("small", NS, dict(T=3, U=3, A=4, S=2, entry="loss"))] + \
            [(t, ns, dict(f, S=2, entry="loss")) for t, ns, f in _stats_rows(d, kw=lambda a: {})]
    if lib == "joiner":                # no sample loop: N itself on grid.x (joiner_prep_kernel), and past 65535 samples the
        acts = ("identity", "relu", "tanh")                 # two-pass backward in the single pass's place (jn_plan)
        return [("l%d" % lay, NS, dict(layout=lay, act=acts[(i + lay) % 3], T=2, U=3, H=4, S=2 if lay == 2 else 0))
                for lay in (0, 1, 2)]
    if lib in ("mi", "bestpath"):
        return [("small_%s" % "rm"[m], (NS[(i + m) % 2],), dict(S=2, T=3, mod=bool(m))) for m in (0, 1)] + \
            [("u65_%s" % "rm"[m], NS[1:], dict(S=64, T=2, mod=bool(m))) for m in (0, 1)]
    raise KeyError(lib)


LIBS = ("tdt", "mblank", "mono", "ar", "delay", "pstream", "pruned", "hat", "kd", "mi", "bestpath", "tdt_align")
WHOLE_N_LIBS = ("joiner",)             # rows of the same make for the launches with N itself on a grid dimension


def _rows():
    rows = {}
    for lib in LIBS + WHOLE_N_LIBS:
        for i, d in enumerate(DTYPES):
            for tag, ns, fields in _variants(lib, d, i):
                for n in ns:
                    name = "%s_%s_%s_n%d" % (lib, d, tag, n)
                    rows[name] = dict(name=name, lib=lib, dtype=d, N=n, **fields)
    return rows


ROWS = _rows()

# Sliced kernels (library, base name) whose entry refuses N > 65535 before the sample loop can take a second slice.
REFUSED = {
    ("pruned", "pruned_window_kernel"):
        "compute_rnnt_prune_ranges_add runs the additive joint's partition kernels, which keep the samples on one grid "
        "dimension: run_prune_ranges refuses N > 65535 (INVALID_VALUE, include/rnnt_pruned.h: BATCH SIZE); "
        "tests/test_gpu_side_limits.py tests the refusal",
}
# What the rows leave out, with why.
NOT_BUILT = {
}


def block_case(row):
    """The forms-table case of a row's base block: N = K samples under the row's name."""
    c = {k: v for k, v in row.items() if k != "lib"}
    c["N"] = K
    return c


def full_case(row):
    return {k: v for k, v in row.items() if k != "lib"}


def slices(row):
    return -(-row["N"] // GRID_SAMPLES)


def kernels(row, cus=256):
    """The sliced kernels (full names) the library's release rules launch for a row: each runs slices(row) times per call.
    A library without a sample loop (the joiner): every kernel of the row, each launched once."""
    F = forms_of(row["lib"])
    if row["lib"] in WHOLE_N_LIBS:
        return {k for ks in F.predict(full_case(row), cus).values() for k in ks}
    return {k for ks in F.predict(full_case(row), cus).values() for k in ks if k.split("<")[0].split("::")[-1] in ALL_SLICED}


def elements(row):
    """Elements of a row's largest tensor."""
    n = row["N"]
    if "H" in row:
        return n * row["T"] * row["U"] * row["H"]
    if "mod" in row:
        return n * (row["S"] + 1) * (row["T"] + 1)
    width = row["A"] + (len(row["durations"]) if "durations" in row and "columns" not in row else 0)
    return n * row["T"] * row.get("S", row["U"]) * width


def covered(lib):
    """{object: set of sliced kernels} the rows of a library reach."""
    out = {}
    for r in ROWS.values():
        if r["lib"] == lib:
            out.setdefault(STORES[r["dtype"]][0], set()).update(kernels(r))
    return out


# ----------------------------------------------------------------------------- the capped grids
ELEM_BLOCKS, ELEM_THREADS = 65536, 256          # elem_grid (csrc/rnnt_side_host.h)
TRIPS = {
    "elem_grid": dict(cap=ELEM_BLOCKS, per_block={"*": ELEM_THREADS},
                      users={"tdt": "tdt_grad_elem_kernel", "mblank": "mblank_grad_elem_kernel", "hat": "hat_grad_elem_kernel",
                             "kd": "kd_grad_elem_kernel", "pruned": "pruned_grad_elem_kernel"}),
    # joiner_fwd_kernel: rows = N T J, 256 / PX rows per block (PX = the packets of a row of H, rounded up to a power of two,
    # at most 256); joiner_df_kernel / joiner_dg_kernel: N T / N U rows at the same rows per block; joiner_dg_sum_kernel:
    # 256 elements per block of E = N U H
    "jn_row_grid": dict(cap=1 << 20, per_block={"joiner_fwd_kernel": "256 / PX", "joiner_df_kernel": "256 / PX",
                                                "joiner_dg_kernel": "256 / PX", "joiner_dg_sum_kernel": 256},
                        users={"joiner": ("joiner_fwd_kernel", "joiner_df_kernel", "joiner_dg_kernel", "joiner_dg_sum_kernel")}),
    # logprobs_edges_kernel: 256 cells per block of B U (T + 1 - mod); logprobs_grad_kernel: 256 / PX rows per block of
    # B T K' rows.  (logprobs_lse_kernel's grid is not capped: (rows G + 255) / 256 blocks.)
    "lp_grid": dict(cap=1 << 20, per_block={"logprobs_edges_kernel": 256, "logprobs_grad_kernel": "256 / PX"},
                    users={"logprobs": ("logprobs_edges_kernel", "logprobs_grad_kernel")}),
}
UNREACHABLE = {
    ("joiner", "joiner_dg_sum_kernel"):
        "launched only on the single-pass route with TZ > 1 shares: jn_shares needs N ceil(H / 64) < 1024, so N H < 65536, and "
        "the single pass needs U comp 64 <= 64 KB, so U <= 256: E = N U H < 2^24, below the 2^20 x 256 = 2^28 elements of "
        "one trip",
}


def _elem_fields(lib, d, mode=1):
    A = 140009                                   # odd, large: few rows, so that the fp64 reference takes seconds
    base = dict(T=6, U=5, A=A, off=STORES[d][3])
    if lib == "tdt":
        return dict(base, durations=(0, 1))
    if lib == "mblank":
        return dict(base, blank=A - 1, columns=(A // 2,), durations=(2,))
    if lib == "hat":
        return dict(base, blank=A // 3)
    if lib == "kd":
        return dict(base, blank=A // 3, mode=mode, toff=0)
    if lib == "pruned":          # N = 3: from four samples on, the module's windows give the last sample no path
        return dict(base, N=3, T=8, U=6, S=5, entry="loss")
    raise KeyError(lib)


def _trip_rows():
    rows = {}
    for lib in TRIPS["elem_grid"]["users"]:
        for d in DTYPES:
            for mode in ((0, 1) if lib == "kd" else (1,)):      # kd: the kernel is instantiated per mode
                name = "elem_%s_%s%s" % (lib, d, "_m0" if mode == 0 else "")
                # every sample full length: element 2^24 lies in the last one
                f = dict(dict(N=4), **_elem_fields(lib, d, mode))
                rows[name] = dict(name=name, lib=lib, dtype=d, grid="elem_grid",
                                  lengths=((f["T"],) * f["N"], (f["U"] - 1,) * f["N"]), **f)
    return rows


TRIP_ROWS = _trip_rows()


def trip_elements(row):
    """E of an elem_grid row: the elements of the logits."""
    return elements(row)


def trips(row):
    """Trips of the grid-stride loop a row's capped kernel takes."""
    g = TRIPS[row["grid"]]
    return -(-trip_elements(row) // (g["cap"] * g["per_block"]["*"]))


def trip_boundary(row):
    """(sample, row of the sample, column) of the first element of the second trip."""
    g = TRIPS[row["grid"]]
    e = g["cap"] * g["per_block"]["*"]
    per_row = elements(dict(row, N=1)) // (row["T"] * row.get("S", row["U"]))
    r, col = divmod(e, per_row)
    return divmod(r, row["T"] * row.get("S", row["U"])) + (col,)


def trip_kernel(row):
    F = forms_of(row["lib"])
    want = TRIPS[row["grid"]]["users"][row["lib"]]
    ks = {k for ks in F.predict(full_case(row), 256).values() for k in ks if k.split("<")[0].split("::")[-1] == want}
    assert len(ks) == 1, (row["name"], ks)
    return next(iter(ks))


# ----------------------------------------------------------------------------- the logprobs grid
LP_CAP = TRIPS["lp_grid"]["cap"]


def lp_px(row):
    """Threads along a row in logprobs_grad_kernel (run_logprobs_bwd): the packets of a row rounded up to a power of two."""
    e = STORES[row["dtype"]][3]
    v = 16 // e if (row["C"] * e) % 16 == 0 else 1
    p = row["C"] // v
    return min(1 << max(p - 1, 0).bit_length(), 256)


def lp_work(row):
    """{kernel base name: (work items, items per block)}: cells of px / py for the edges kernel, rows of logits for the gradient."""
    B, T, U, mod = row["B"], row["T"], row["U"], row["mod"]
    return {"logprobs_edges_kernel": (B * U * (T + 1 - mod), 256), "logprobs_grad_kernel": (B * T * U, 256 // lp_px(row))}


def lp_trips(row):
    return {k: -(-work // (LP_CAP * per)) for k, (work, per) in lp_work(row).items()}


def lp_bytes(row):
    """Peak device bytes: logits and dlogits, lse, px, py and the two gradients in the lattice type, one fp64 slab of 2^24 rows."""
    e, lat = STORES[row["dtype"]][3], 8 if row["dtype"] == "f64" else 4
    rows = row["B"] * row["T"] * row["U"]
    return 2 * rows * row["C"] * e + 5 * (rows + row["B"] * row["U"]) * lat + 4 * (1 << 24) * row["C"] * 8


def _lp_rows():
    rows = {}
    # joint form (K = 0), one sample, U = 2: rows = 2 T = 2^28 + 8; C: a row shorter than a packet (element-wise gradient
    # form, 128 rows per block) and a row of one packet (the vector form, 256 rows per block)
    # (fp64: 3 columns, 24 bytes, for the element-wise form -- 64 rows per block; 2 columns are one packet)
    for d, cs in (("f32", (2, 4)), ("f64", (3, 2)), ("bf16", (2, 8))):
        for c in cs:
            name = "lp_%s_c%d" % (d, c)
            rows[name] = dict(name=name, lib="logprobs", dtype=d, grid="lp_grid", K=0, mod=0, B=1, T=(1 << 27) + 4, U=2, C=c)
    return rows


LP_ROWS = _lp_rows()


# ----------------------------------------------------------------------------- the joiner's row grid
JN_CAP = TRIPS["jn_row_grid"]["cap"]
JN_KERNELS = ("joiner_fwd_kernel", "joiner_df_kernel", "joiner_dg_kernel")


def jn_px(row):
    """Threads along a row (jn_plan): the packets of a row of H rounded up to a power of two, at most 256."""
    e = STORES[row["dtype"]][3]
    v = 16 // e if (row["H"] * e) % 16 == 0 else 1
    p = row["H"] // v
    return min(1 << max(p - 1, 0).bit_length(), 256)


def jn_work(row):
    """{kernel base name: (rows, rows per block)}: rows of out, of df and of dg (padded layout: J = U)."""
    N, T, U = row["N"], row["T"], row["U"]
    per = 256 // jn_px(row)
    return {"joiner_fwd_kernel": (N * T * U, per), "joiner_df_kernel": (N * T, per), "joiner_dg_kernel": (N * U, per)}


def jn_trips(row):
    return {k: -(-work // (JN_CAP * per)) for k, (work, per) in jn_work(row).items()}


def jn_bytes(row):
    """Peak device bytes: out, dout, torch's own out, f or g and df or dg of the same size, one fp64 slab of 4096 samples."""
    e = STORES[row["dtype"]][3]
    big = row["N"] * row["T"] * row["U"] * row["H"]
    return 5 * big * e + 2 * row["N"] * row["H"] * e + 4 * 4096 * row["T"] * row["U"] * row["H"] * 8


def _jn_rows():
    """Padded layout, every sample full length, N = 65537 (past 65535 samples the backward is joiner_df_kernel +
    joiner_dg_kernel).  f-heavy (T = 4097, U = 1): N T = 2^28 + 2^16 + 4097 rows of out and of df; g-heavy (T = 1, U = 4097):
    as many rows of out and of dg.  H: one 16-byte packet (the vector form) or one element (the element-wise form), both one
    thread along the row, 256 rows per block."""
    rows = {}
    for d in DTYPES:
        e = STORES[d][3]
        for form, H, act in (("vec", 16 // e, "relu"), ("elem", 1, "identity")):
            for heavy, T, U in (("f", 4097, 1), ("g", 1, 4097)):
                name = "jn_%s_%s_%s" % (d, form, heavy)
                rows[name] = dict(name=name, lib="joiner", dtype=d, grid="jn_row_grid", layout=0, act=act, N=65537, T=T, U=U,
                                  H=H, S=0, full=True, heavy=heavy)
    return rows


JN_ROWS = _jn_rows()


def jn_kernels(row):
    """The kernels (full names) a row takes into a second trip."""
    F = forms_of("joiner")
    trips = jn_trips(row)
    case = {k: v for k, v in row.items() if k not in ("lib", "grid", "heavy")}
    return {k for ks in F.predict(case).values() for k in ks if trips.get(k.split("<")[0].split("::")[-1], 0) >= 2}


def row_seed(row):
    return zlib.crc32(row["name"].encode())
