"""The kernel forms of libwarprnnt_ar.so (csrc/rnnt_ar.hip, rnnt_ar_f64.hip, rnnt_ar_h16.hip): which kernels its three code
objects hold, the release rules that pick them (a restatement of run_ar / launch_ar_stats / launch_ar_lattice,
csrc/rnnt_ar_impl.h, and of launch_mblank_grad, csrc/rnnt_mblank_impl.h, whose K = 0 gradient stream this library launches),
and the cases that reach every form -- the counterpart of tests/mono_forms.py.  tests/test_ar_cpu.py checks the table against
the built code objects; tests/test_gpu_ar.py runs every case and checks that exactly the predicted kernels ran.

A case: dtype, N, T (= maxT), U (= maxU), A, blank; `off` = byte offset of the logits and gradients from a 16-byte boundary
(the element-wise gradient form).  Lengths come from `lengths(case, rng)`, windows from `windows(case, tl, ll, rng)`."""
import numpy as np

from tests import ar_ref as R
from tests import forms_common as C
from tests.forms_common import STORES, object_of, stats_group           # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_ar.hip", "f64": "rnnt_ar_f64.hip", "h16": "rnnt_ar_h16.hip"}
STAGES = ("bounds", "stats", "lattice", "coef", "grad")
CHUNK = 8               # kArChunk: diagonals per chunk of the wave form
WAVE_MAX_U = 64         # kArWaveMaxU: the release rule of the lattice
PINNED, UNRESTRICTED = 3, 4     # the samples of a batch with every label pinned / with unrestricted windows


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"ar_bounds_kernel": "bounds", "ar_stats_kernel": "stats", "ar_lattice_wave_kernel": "lattice",
            "ar_lattice_block_kernel": "lattice", "ar_coef_kernel": "coef", "mblank_grad_kernel": "grad",
            "mblank_grad_elem_kernel": "grad"}.get(base)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` (no rule depends on the compute-unit count)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    form = "wave" if case["U"] <= WAVE_MAX_U else "block"
    return {"bounds": {"rnnt::ar_bounds_kernel<%s>" % lat},
            "stats": {"rnnt::ar_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {"rnnt::ar_lattice_%s_kernel<%s>" % (form, lat)},
            "coef": {"rnnt::ar_coef_kernel<%s>" % lat},
            "grad": {"rnnt::mblank_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::mblank_grad_elem_kernel<%s>" % tag}}


def lengths(case, rng):
    """(T_b, L_b) of a case's batch.  Sample 0 is full (T, U - 1); then, as far as N reaches: one sample with T_b = 1, one
    with L_b = 0, the sample whose labels `windows` pins (at least one label where U allows) and the one it leaves
    unrestricted (likewise); the rest random."""
    N, T, U = case["N"], case["T"], case["U"]
    tl = rng.integers(1, T + 1, size=N)
    ll = rng.integers(0, U, size=N)
    tl[0], ll[0] = T, U - 1
    if N > 1:
        tl[1] = 1
    if N > 2:
        ll[2] = 0
    for b in (PINNED, UNRESTRICTED):
        if N > b and U > 1:
            ll[b] = rng.integers(1, U)
            tl[b] = rng.integers(min(2, T), T + 1)
    return tl.astype(np.int32), ll.astype(np.int32)


def windows(case, tl, ll, rng):
    """(emit_lo, emit_hi) of a case's batch (tests/ar_ref.py windows): feasible throughout, sample PINNED with a single
    path, sample UNRESTRICTED with windows that restrict nothing."""
    lo, hi, _ = R.windows(rng, tl, ll, case["U"], pinned=(PINNED,), unrestricted=(UNRESTRICTED,))
    return lo, hi


def _case(name, dtype, N, T, U, A, blank, **kw):
    assert 0 <= blank < A and (N >= 5 or name.endswith("u1100"))
    return dict(name=name, dtype=dtype, N=N, T=T, U=U, A=A, blank=blank, **kw)


def _cases():
    cs = []
    for d in ("f32", "f64", "bf16", "f16"):
        esz = STORES[d][3]
        lo, hi = 256 // esz, 2048 // esz                      # the last row widths of 4 and of 16 lanes per row
        cs += [_case("%s_a%d" % (d, lo), d, 5, 9, 7, lo, lo - 1),
               _case("%s_a%d" % (d, lo + 1), d, 5, 8, 6, lo + 1, 0),
               _case("%s_a%d" % (d, hi), d, 5, 7, 5, hi, hi // 2),
               _case("%s_a%d" % (d, hi + 1), d, 5, 7, 5, hi + 1, hi),
               # off the 16-byte boundary: the element-wise gradient
               _case(d + "_off", d, 5, 7, 5, 63, 62, off=esz)]
    # A = 3 .. 7: packets straddle rows
    for A, d in ((3, "f32"), (4, "bf16"), (5, "f64"), (6, "f16"), (7, "f32")):
        cs.append(_case("%s_a%d" % (d, A), d, 6, 9, 6, A, (0, A - 1, A // 2)[A % 3]))
    for d in ("f32", "f64"):
        # the wave form: one column, two columns, every lane live (L_0 = 63)
        cs += [_case(d + "_u1", d, 5, 6, 1, 5, 2), _case(d + "_u2", d, 5, 6, 2, 5, 0), _case(d + "_u64", d, 5, 10, 64, 5, 4)]
        # T + U of the full sample at one chunk of the wave form minus one, exactly one chunk and one more; three chunks.  The
        # sweep takes T + U - 1 steps (diagonals), so CHUNK + 2 and 3 CHUNK + 1 put the step count itself past a chunk's end
        for TU in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 3 * CHUNK, 3 * CHUNK + 1):
            cs.append(_case("%s_tu%d" % (d, TU), d, 5, TU - 4, 4, 9, 8))
        # the block form: its first width, more than two wavefronts, and every thread of a full block with two columns
        cs += [_case(d + "_u65", d, 5, 9, 65, 5, 0), _case(d + "_u130", d, 5, 12, 130, 6, 5),
               _case(d + "_u1100", d, 2, 5, 1100, 4, 3)]
    # the block form from 16-bit storage (the fp32 lattice kernels of the third code object)
    cs.append(_case("bf16_u65", "bf16", 5, 9, 65, 8, 7))
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
