"""The kernel forms of libwarprnnt_mono.so (csrc/rnnt_mono.hip, rnnt_mono_f64.hip, rnnt_mono_h16.hip): which kernels its three
code objects hold, the release rules that pick them (a restatement of run_mono / launch_mono_stats / launch_mono_lattice,
csrc/rnnt_mono_impl.h, and of launch_mblank_grad, csrc/rnnt_mblank_impl.h, whose K = 0 gradient stream this library
launches), and the cases that reach every form -- the counterpart of tests/mblank_forms.py.  tests/test_mono_cpu.py checks
the table against the built code objects; tests/test_gpu_mono.py runs every case and checks that exactly the predicted
kernels ran.

A case: dtype, N, T (= maxT), U (= maxU), A, blank; `off` = byte offset of the logits and gradients from a 16-byte boundary
(the element-wise gradient form).  Lengths come from `lengths(case, rng)`, always with T_b >= L_b."""
import numpy as np

from tests import forms_common as C
from tests.forms_common import STORES, object_of, stats_group           # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_mono.hip", "f64": "rnnt_mono_f64.hip", "h16": "rnnt_mono_h16.hip"}
STAGES = ("stats", "lattice", "coef", "grad")
CHUNK = 8               # kMonoChunk: frames per chunk of the wave form
WAVE_MAX_U = 64         # kMonoWaveMaxU: the release rule of the lattice


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"mono_stats_kernel": "stats", "mono_lattice_wave_kernel": "lattice", "mono_lattice_block_kernel": "lattice",
            "mono_coef_kernel": "coef", "mblank_grad_kernel": "grad", "mblank_grad_elem_kernel": "grad"}.get(base)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` (no rule depends on the compute-unit count)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    form = "wave" if case["U"] <= WAVE_MAX_U else "block"
    return {"stats": {"rnnt::mono_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {"rnnt::mono_lattice_%s_kernel<%s>" % (form, lat)},
            "coef": {"rnnt::mono_coef_kernel<%s>" % lat},
            "grad": {"rnnt::mblank_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::mblank_grad_elem_kernel<%s>" % tag}}


def lengths(case, rng):
    """(T_b, L_b) of a case's batch, every T_b >= L_b.  Sample 0 is full (T, min(U - 1, T)); then, as far as N reaches:
    one sample with T_b = 1, one with L_b = 0, one with T_b = L_b (a single path), one with T_b = L_b + 1; the rest random."""
    N, T, U = case["N"], case["T"], case["U"]
    ll = rng.integers(0, min(U - 1, T) + 1, size=N)
    tl = np.array([rng.integers(max(int(l), 1), T + 1) for l in ll])
    tl[0], ll[0] = T, min(U - 1, T)
    if N > 1:
        tl[1], ll[1] = 1, min(int(rng.integers(0, 2)), U - 1)
    if N > 2:
        ll[2] = 0
    if N > 3 and U > 1:
        ll[3] = rng.integers(1, min(U - 1, T) + 1)
        tl[3] = ll[3]
    if N > 4:
        ll[4] = rng.integers(0, min(U - 1, T - 1) + 1)
        tl[4] = ll[4] + 1
    assert (tl >= ll).all() and (tl >= 1).all() and (tl <= T).all() and (ll <= U - 1).all()
    return tl.astype(np.int32), ll.astype(np.int32)


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
               _case(d + "_off", d, 5, 6, 5, 63, 62, off=esz),
               # a second round of the row reduction (csrc/rnnt_row_lse.h: more than 4 G packets) at 4 and at 64 lanes per row:
               # 256-byte rows one element off the boundary, 17 packets each; rows just past 4096 bytes, 257 packets or more
               _case("%s_a%d_off" % (d, lo), d, 5, 6, 5, lo, 1, off=esz),
               _case("%s_a%d" % (d, 2 * hi + 1), d, 5, 5, 4, 2 * hi + 1, 2 * hi)]
    # A = 3 .. 7: packets straddle rows
    for A, d in ((3, "f32"), (4, "bf16"), (5, "f64"), (6, "f16"), (7, "f32")):
        cs.append(_case("%s_a%d" % (d, A), d, 6, 9, 6, A, (0, A - 1, A // 2)[A % 3]))
    for d in ("f32", "f64"):
        # the wave form: one column, two columns, every lane live (L_0 = 63)
        cs += [_case(d + "_u1", d, 5, 6, 1, 5, 2), _case(d + "_u2", d, 5, 6, 2, 5, 0), _case(d + "_u64", d, 5, 70, 64, 5, 4)]
        # one chunk of the wave form minus, exactly and plus one frame; three chunks (two re-centrings)
        for T in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 4):
            cs.append(_case("%s_t%d" % (d, T), d, 5, T, 5, 9, 8))
        # the block form: its first width, more than two wavefronts, and every thread of a full block with two columns
        cs += [_case(d + "_u65", d, 5, 70, 65, 5, 0), _case(d + "_u130", d, 5, 140, 130, 6, 5),
               _case(d + "_u1100", d, 2, 1101, 1100, 4, 3)]
    # the block form from 16-bit storage (the fp32 lattice kernels of the third code object)
    cs.append(_case("bf16_u65", "bf16", 5, 70, 65, 8, 7))
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
