"""The kernel forms of libwarprnnt_pstream.so (csrc/rnnt_pstream.hip, rnnt_pstream_f64.hip, rnnt_pstream_h16.hip): which
kernels its three code objects hold, the release rules that pick them (a restatement of run_pstream / launch_pstream_stats /
launch_pstream_lattice, csrc/rnnt_pstream_impl.h, and of launch_mblank_grad, csrc/rnnt_mblank_impl.h, whose K = 0 gradient
stream this library launches over its compact record table), and the cases that reach every form -- the counterpart of
tests/delay_forms.py.  tests/test_pstream_cpu.py checks the table against the built code objects; tests/test_gpu_pstream.py
runs every case and checks that exactly the predicted kernels ran.

A case: dtype, N, T (= maxT), U (= maxU), S (rows per frame), A, blank, type (0 regular, 1 modified); `off` = byte offset of
the logits and gradients from a 16-byte boundary (the element-wise gradient form); `burst`: windows whose starts jump by
S - 1.  Lengths come from `lengths(case, rng)`, window starts from `ranges(case, tl, ll, rng)`."""
import numpy as np

from tests import forms_common as C
from tests import pstream_ref as R
from tests.forms_common import STORES, object_of, stats_group           # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_pstream.hip", "f64": "rnnt_pstream_f64.hip", "h16": "rnnt_pstream_h16.hip"}
STAGES = ("prep", "stats", "lattice", "close", "coef", "grad")
AR_CHUNK, AR_WAVE_MAX_U = 8, 64         # kArChunk, kArWaveMaxU: the regular lattice (csrc/rnnt_ar_kernels.h)
MONO_CHUNK, MONO_WAVE_MAX_U = 8, 64     # kMonoChunk, kMonoWaveMaxU: the modified lattice (csrc/rnnt_mono_kernels.h)
FRAME_ZERO = 3          # the sample of a batch with T_b = 1 and L_b >= 1 where the windows allow a label in one frame
LATTICE = {0: "ar", 1: "mono"}


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"pstream_prep_kernel": "prep", "pstream_stats_kernel": "stats", "ar_lattice_wave_kernel": "lattice",
            "ar_lattice_block_kernel": "lattice", "mono_lattice_wave_kernel": "lattice", "mono_lattice_block_kernel": "lattice",
            "pstream_close_kernel": "close", "pstream_coef_kernel": "coef", "mblank_grad_kernel": "grad",
            "mblank_grad_elem_kernel": "grad"}.get(base)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` with gradients (no rule depends on the compute-unit
    count)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    wave_max = MONO_WAVE_MAX_U if case["type"] else AR_WAVE_MAX_U
    form = "wave" if case["U"] <= wave_max else "block"
    return {"prep": {"rnnt::pstream_prep_kernel<%s>" % lat},
            "stats": {"rnnt::pstream_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {"rnnt::%s_lattice_%s_kernel<%s>" % (LATTICE[case["type"]], form, lat)},
            "close": {"rnnt::pstream_close_kernel<%s>" % lat},
            "coef": {"rnnt::pstream_coef_kernel<%s>" % lat},
            "grad": {"rnnt::mblank_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::mblank_grad_elem_kernel<%s>" % tag}}


def lengths(case, rng):
    """(T_b, L_b) of a case's batch, as tests/delay_forms.py's: sample 0 full (T, U - 1); then, as far as N reaches, one
    sample with T_b = 1, one with L_b = 0 and one with T_b = 1 and L_b >= 1; the rest random -- with every L_b capped at
    what windows of S states over T_b frames can hold (pstream_ref.max_labels: T_b in the modified type, T_b (S - 1) in the
    regular one), so that every sample has a path."""
    N, T, U, S, typ = case["N"], case["T"], case["U"], case["S"], case["type"]
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
    ll = np.minimum(ll, [R.max_labels(int(t), S, typ) for t in tl])
    return tl.astype(np.int32), ll.astype(np.int32)


def ranges(case, tl, ll, rng):
    """(N, T) int32 window starts around a valid path of every sample (pstream_ref.windows)."""
    return np.stack([R.windows(rng, int(tl[b]), int(ll[b]), case["S"], case["type"], case["T"], case.get("burst", False))
                     for b in range(case["N"])])


def _case(name, dtype, typ, N, T, U, S, A, blank, **kw):
    assert 0 <= blank < A and 1 <= S <= U and typ in (0, 1) and (N >= 5 or "u1100" in name)
    # sample 0 is full: L_0 = U - 1 labels fit the windows (but in the regular type at S = 1, which holds no label at all)
    assert U - 1 <= R.max_labels(T, S, typ) or (typ == 0 and S == 1), name
    return dict(name=name, dtype=dtype, type=typ, N=N, T=T, U=U, S=S, A=A, blank=blank, **kw)


def _cases():
    cs = []
    for i, d in enumerate(("f32", "f64", "bf16", "f16")):
        esz = STORES[d][3]
        lo, hi = 256 // esz, 2048 // esz                      # the last row widths of 4 and of 16 lanes per row
        a, b = i % 2, (i + 1) % 2                             # both lattice types from every code object
        cs += [_case("%s_a%d" % (d, lo), d, a, 5, 9, 7, 3, lo, lo - 1),
               _case("%s_a%d" % (d, lo + 1), d, b, 5, 8, 6, 2, lo + 1, 0),
               _case("%s_a%d" % (d, hi), d, a, 5, 7, 5, 4, hi, hi // 2),
               _case("%s_a%d" % (d, hi + 1), d, b, 5, 7, 5, 2, hi + 1, hi),
               # off the 16-byte boundary: the element-wise gradient
               _case(d + "_off", d, a, 5, 7, 5, 3, 63, 62, off=esz)]
    # A = 3 .. 7: packets straddle rows
    for A, d in ((3, "f32"), (4, "bf16"), (5, "f64"), (6, "f16"), (7, "f32")):
        cs.append(_case("%s_a%d" % (d, A), d, A % 2, 6, 9, 6, 3, A, (0, A - 1, A // 2)[A % 3]))
    # the windows: one state per frame (the regular type then holds no label: every L_b = 0), two, the whole lattice (the
    # materialised tensor), five of twenty-one; starts that jump by S - 1
    for typ in (0, 1):
        n = "f32_t%d_" % typ
        cs += [_case(n + "s1", "f32", typ, 5, 8, 6, 1, 9, 8), _case(n + "s2", "f32", typ, 5, 9, 7, 2, 9, 0),
               _case(n + "sU", "f32", typ, 5, 9, 6, 6, 9, 4), _case(n + "s5_u21", "f32", typ, 6, 24, 21, 5, 11, 10),
               _case(n + "burst", "f32", typ, 5, 12, 13, 4, 9, 2, burst=True)]
    for d in ("f32", "f64"):
        for typ in (0, 1):
            n = "%s_t%d_" % (d, typ)
            tt = lambda U: U + 2 if typ else max(4, (U + 1) // 2)               # noqa: E731  (frames that hold U - 1 labels at S = 3)
            # the wave form: one column, two columns, every lane live (L_0 = 63); the block form: its first width, more
            # than two wavefronts, and every thread of a full block with two columns
            cs += [_case(n + "u1", d, typ, 5, 6, 1, 1, 5, 2), _case(n + "u2", d, typ, 5, 6, 2, 2, 5, 0),
                   _case(n + "u64", d, typ, 5, tt(64), 64, 3, 5, 4), _case(n + "u65", d, typ, 5, tt(65), 65, 3, 5, 0),
                   _case(n + "u66", d, typ, 5, tt(66), 66, 3, 5, 1), _case(n + "u130", d, typ, 5, tt(130), 130, 3, 6, 5),
                   _case(n + "u1100", d, typ, 2, 1101 if typ else 560, 1100, 2 if typ else 3, 4, 3)]
            # the full sample's sweep around a chunk of the wave form.  Regular: T + U at one short of a chunk, a chunk, one
            # more, three chunks and one more; the sweep takes T + U - 1 steps (diagonals), so chunk + 2 and 3 chunk + 2 put
            # the step count itself past a chunk's end.  Modified: the sweep takes T steps (frames)
            if typ:
                for T in (MONO_CHUNK - 1, MONO_CHUNK, MONO_CHUNK + 1, 3 * MONO_CHUNK, 3 * MONO_CHUNK + 1):
                    cs.append(_case("%st%d" % (n, T), d, typ, 5, T, 4, 2, 9, 8))
            else:
                for TU in (AR_CHUNK - 1, AR_CHUNK, AR_CHUNK + 1, AR_CHUNK + 2, 3 * AR_CHUNK, 3 * AR_CHUNK + 1, 3 * AR_CHUNK + 2):
                    cs.append(_case("%stu%d" % (n, TU), d, typ, 5, TU - 4, 4, 2, 9, 8))
    # the block form from 16-bit storage (the fp32 lattice kernels of the third code object), both types
    for typ in (0, 1):
        cs += [_case("bf16_t%d_u65" % typ, "bf16", typ, 5, 67, 65, 3, 8, 7), _case("f16_t%d_u65" % typ, "f16", typ, 5, 67, 65, 4, 8, 0)]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
