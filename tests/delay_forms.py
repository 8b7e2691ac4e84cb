"""The kernel forms of libwarprnnt_delay.so (csrc/rnnt_delay.hip, rnnt_delay_f64.hip, rnnt_delay_h16.hip): which kernels its
three code objects hold, the release rules that pick them (a restatement of run_delay / launch_delay_stats /
launch_delay_lattice / launch_delay_emit, csrc/rnnt_delay_impl.h, and of launch_mblank_grad, csrc/rnnt_mblank_impl.h, whose
K = 0 gradient stream this library launches), and the cases that reach every form -- the counterpart of tests/ar_forms.py.
tests/test_delay_cpu.py checks the table against the built code objects; tests/test_gpu_delay.py runs every case with
emit_frames and checks that exactly the predicted kernels ran.

A case: dtype, N, T (= maxT), U (= maxU), A, blank; `off` = byte offset of the logits and gradients from a 16-byte boundary
(the element-wise gradient form).  Lengths come from `lengths(case, rng)`."""
import numpy as np

from tests import forms_common as C
from tests.forms_common import STORES, object_of, stats_group           # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_delay.hip", "f64": "rnnt_delay_f64.hip", "h16": "rnnt_delay_h16.hip"}
STAGES = ("stats", "lattice", "coef", "emit", "grad")
CHUNK = 8               # kArChunk: diagonals per chunk of the wave form
WAVE_MAX_U = 64         # kArWaveMaxU: the release rule of the lattice
EMIT_SLICES = 8         # kDelayEmitSlices: frame slices of the narrow emission form (32 lanes across u)
EMIT_NARROW = 64        # kDelayEmitNarrow: label columns (maxU - 1) up to which the emission kernel slices the frames
FRAME_ZERO = 3          # the sample of a batch with T_b = 1 and L_b >= 1: every label at frame 0


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"delay_stats_kernel": "stats", "ar_lattice_wave_kernel": "lattice", "ar_lattice_block_kernel": "lattice",
            "delay_coef_kernel": "coef", "delay_emit_kernel": "emit", "mblank_grad_kernel": "grad",
            "mblank_grad_elem_kernel": "grad"}.get(base)


def emit_slices(U):
    """launch_delay_emit: frame slices per block (None: maxU == 1, no label column, no launch)."""
    return None if U == 1 else EMIT_SLICES if U - 1 <= EMIT_NARROW else 1


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` with gradients and emit_frames (no rule depends on
    the compute-unit count)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    form = "wave" if case["U"] <= WAVE_MAX_U else "block"
    s = emit_slices(case["U"])
    return {"stats": {"rnnt::delay_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {"rnnt::ar_lattice_%s_kernel<%s>" % (form, lat)},
            "coef": {"rnnt::delay_coef_kernel<%s>" % lat},
            "emit": set() if s is None else {"rnnt::delay_emit_kernel<%s, %d>" % (lat, s)},
            "grad": {"rnnt::mblank_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::mblank_grad_elem_kernel<%s>" % tag}}


def lengths(case, rng):
    """(T_b, L_b) of a case's batch.  Sample 0 is full (T, U - 1); then, as far as N reaches: one sample with T_b = 1, one
    with L_b = 0 and one with T_b = 1 and L_b >= 1 (where U allows: every label at frame 0); the rest random."""
    N, T, U = case["N"], case["T"], case["U"]
    tl = rng.integers(1, T + 1, size=N)
    ll = rng.integers(0, U, size=N)
    tl[0], ll[0] = T, U - 1
    if N > 1:
        tl[1] = 1
    if N > 2:
        ll[2] = 0
    if N > FRAME_ZERO:
        tl[FRAME_ZERO] = 1
        if U > 1:
            ll[FRAME_ZERO] = rng.integers(1, U)
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
               _case(d + "_off", d, 5, 7, 5, 63, 62, off=esz)]
    # A = 3 .. 7: packets straddle rows
    for A, d in ((3, "f32"), (4, "bf16"), (5, "f64"), (6, "f16"), (7, "f32")):
        cs.append(_case("%s_a%d" % (d, A), d, 6, 9, 6, A, (0, A - 1, A // 2)[A % 3]))
    for d in ("f32", "f64"):
        # the wave form: one column (no emission launch), two columns, every lane live (L_0 = 63)
        cs += [_case(d + "_u1", d, 5, 6, 1, 5, 2), _case(d + "_u2", d, 5, 6, 2, 5, 0), _case(d + "_u64", d, 5, 10, 64, 5, 4)]
        # T + U of the full sample at one chunk of the wave form minus one, exactly one chunk and one more; three chunks.  The
        # sweep takes T + U - 1 steps (diagonals), so CHUNK + 2 and 3 CHUNK + 1 put the step count itself past a chunk's end
        for TU in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 3 * CHUNK, 3 * CHUNK + 1):
            cs.append(_case("%s_tu%d" % (d, TU), d, 5, TU - 4, 4, 9, 8))
        # the block form: its first width, more than two wavefronts, and every thread of a full block with two columns.
        # U = 65 is also the emission kernel's last sliced width (64 label columns, two blocks of 32 lanes), U = 66 its
        # first with a thread per column
        cs += [_case(d + "_u65", d, 5, 9, 65, 5, 0), _case(d + "_u66", d, 5, 9, 66, 5, 1), _case(d + "_u130", d, 5, 12, 130, 6, 5),
               _case(d + "_u1100", d, 2, 5, 1100, 4, 3)]
    # the block form from 16-bit storage (the fp32 lattice kernels of the third code object), both emission forms
    cs += [_case("bf16_u65", "bf16", 5, 9, 65, 8, 7), _case("f16_u66", "f16", 5, 9, 66, 8, 0)]
    # the emission kernel's own boundaries.  Sliced form: 32 and 33 label columns (one block, two blocks); T = 40 gives
    # slices of five frames (one round of four requests and a tail), T = 8 one frame per slice, T = 9 two frames per slice
    # and three empty slices.  A thread per column: 256 and 257 label columns (one block, two blocks), T = 40 ten rounds
    cs += [_case("f32_u33_t40", "f32", 5, 40, 33, 5, 0), _case("f32_u34", "f32", 5, 8, 34, 5, 4),
           _case("f64_u34_t9", "f64", 5, 9, 34, 5, 2), _case("f32_u70_t40", "f32", 5, 40, 70, 5, 3),
           _case("f32_u257", "f32", 5, 6, 257, 4, 0), _case("f32_u258", "f32", 5, 6, 258, 4, 1)]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
