"""The kernel forms of libwarprnnt_mblank.so (csrc/rnnt_mblank.hip, rnnt_mblank_f64.hip, rnnt_mblank_h16.hip): which kernels its
three code objects hold, the release rules that pick them (a restatement of run_mblank / launch_mblank_stats /
launch_mblank_grad, csrc/rnnt_mblank_impl.h), and the cases that reach every form -- the counterpart of tests/tdt_forms.py.
tests/test_mblank_cpu.py checks the table against the built code objects; tests/test_gpu_mblank.py runs every case and checks
that exactly the predicted kernels ran.

A case: dtype, N, T, U (= maxU), A, blank, columns and durations of the big blanks; `off` = byte offset of the logits and
gradients from a 16-byte boundary (the element-wise gradient form); `lengths` = (T_b, L_b) when the case needs particular
ones (otherwise gpu_support.ragged_lengths: one sample with T_b = 1 -- every big blank overshoots -- and one with L_b = 0)."""
from tests import forms_common as C
from tests.forms_common import STORES, object_of, stats_group           # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_mblank.hip", "f64": "rnnt_mblank_f64.hip", "h16": "rnnt_mblank_h16.hip"}
STAGES = ("stats", "lattice", "coef", "grad")


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"mblank_stats_kernel": "stats", "mblank_lattice_kernel": "lattice", "mblank_coef_kernel": "coef",
            "mblank_grad_kernel": "grad", "mblank_grad_elem_kernel": "grad"}.get(base)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` (no rule depends on the compute-unit count)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    return {"stats": {"rnnt::mblank_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {"rnnt::mblank_lattice_kernel<%s>" % lat},
            "coef": {"rnnt::mblank_coef_kernel<%s>" % lat},
            "grad": {"rnnt::mblank_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::mblank_grad_elem_kernel<%s>" % tag}}


def nemo_columns(blank, K):
    """NeMo's layout: big blank i in column blank - 1 - i."""
    return tuple(blank - 1 - i for i in range(K))


def _case(name, dtype, N, T, U, A, blank, columns, durations, **kw):
    assert len(columns) == len(durations) and len(set(columns) | {blank}) == len(columns) + 1
    assert all(0 <= c < A for c in columns) and 0 <= blank < A
    return dict(name=name, dtype=dtype, N=N, T=T, U=U, A=A, blank=blank, columns=tuple(columns), durations=tuple(durations),
                **kw)


D8 = (2, 3, 4, 6, 8, 16, 32, 64)


def _cases():
    cs = []
    for d in ("f32", "f64", "bf16", "f16"):
        esz = STORES[d][3]
        lo, hi = 256 // esz, 2048 // esz                      # the last row widths of 4 and of 16 lanes per row
        cs += [
            # K = 3, NeMo's layout, the blank in the last column
            _case("%s_a%d" % (d, lo), d, 4, 9, 7, lo, lo - 1, nemo_columns(lo - 1, 3), (2, 4, 8)),
            # the blank in column 0, big blanks in the first and the last packet of a row and in the middle
            _case("%s_a%d" % (d, lo + 1), d, 3, 8, 6, lo + 1, 0, (1, lo, lo // 2), (2, 3, 5)),
            # the blank in the middle, K = 1
            _case("%s_a%d" % (d, hi), d, 3, 6, 5, hi, hi // 2, (hi - 1,), (2,)),
            # K = 8, the largest duration past every T_b
            _case("%s_a%d" % (d, hi + 1), d, 3, 6, 5, hi + 1, hi, nemo_columns(hi, 8), D8),
            # off the 16-byte boundary: the element-wise gradient
            _case(d + "_off", d, 3, 6, 5, 63, 62, (0, 31), (2, 3), off=esz),
            # K = 0: the plain RNN-T loss
            _case(d + "_k0", d, 4, 7, 5, 21, 10, (), ())]
    # A = 3 .. 7: packets straddle rows
    for A, d, K in ((3, "f32", 1), (4, "bf16", 2), (5, "f64", 3), (6, "f16", 1), (7, "f32", 3)):
        blank = (0, A - 1, A // 2)[A % 3]
        cols = [c for c in range(A) if c != blank][-K:]
        cs.append(_case("%s_a%d" % (d, A), d, 4, 9, 6, A, blank, cols, (2, 3, 4)[:K]))
    # d_max = 64 against T_b = 65, 64 and 63 (the last: the big blank overshoots everywhere); T_b = 1; T_b = 2 = a duration
    for d in ("f32", "f64"):
        cs.append(_case(d + "_d64", d, 6, 65, 4, 9, 8, (7, 6), (2, 64),
                        lengths=((65, 64, 63, 1, 64, 2), (3, 0, 2, 1, 3, 0))))
    # T_b equal to a duration with L_b = 0 (one big blank IS a path); T_b = 1: every big blank overshoots
    cs.append(_case("f32_teq", "f32", 4, 9, 5, 12, 11, nemo_columns(11, 3), (2, 4, 8), lengths=((9, 4, 1, 8), (4, 0, 2, 0))))
    # maxU past one block's thread count: every thread of the lattice block takes two cells of a diagonal
    cs.append(_case("f32_u1100", "f32", 3, 3, 1100, 4, 0, (3,), (2,)))
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
