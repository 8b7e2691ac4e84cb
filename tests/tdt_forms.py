"""The kernel forms of libwarprnnt_tdt.so (csrc/rnnt_tdt.hip, rnnt_tdt_f64.hip, rnnt_tdt_h16.hip): which kernels its three code
objects hold, the release rules that pick them (a restatement of run_tdt / launch_tdt_stats / launch_tdt_grad,
csrc/rnnt_tdt_impl.h), and one case per form that reaches it -- the counterpart of tests/pruned_forms.py.
tests/test_tdt_cpu.py checks the table against the built code objects; tests/test_gpu_tdt.py runs every case and checks that
exactly the predicted kernels ran.

A case: dtype, N, T, U (= maxU), A (token columns), durations; `off` = byte offset of the logits and gradients from a 16-byte
boundary (the element-wise gradient form)."""
from tests import forms_common as C
from tests.forms_common import STORES, object_of, stats_group           # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_tdt.hip", "f64": "rnnt_tdt_f64.hip", "h16": "rnnt_tdt_h16.hip"}
STAGES = ("stats", "lattice", "coef", "grad")


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"tdt_stats_kernel": "stats", "tdt_lattice_kernel": "lattice", "tdt_coef_kernel": "coef",
            "tdt_grad_kernel": "grad", "tdt_grad_elem_kernel": "grad"}.get(base)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` (no rule depends on the compute-unit count)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    return {"stats": {"rnnt::tdt_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {"rnnt::tdt_lattice_kernel<%s>" % lat},
            "coef": {"rnnt::tdt_coef_kernel<%s>" % lat},
            "grad": {"rnnt::tdt_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::tdt_grad_elem_kernel<%s>" % tag}}


def _case(name, dtype, N, T, U, A, durations, **kw):
    return dict(name=name, dtype=dtype, N=N, T=T, U=U, A=A, durations=tuple(durations), **kw)


def _cases():
    cs = []
    for d in ("f32", "f64", "bf16", "f16"):
        cs += [_case(d + "_a5", d, 4, 9, 7, 5, (0, 1, 2, 3, 4)),                   # 4 lanes per row
               _case(d + "_a300", d, 3, 8, 6, 300, (0, 1, 2, 4, 8)),              # 16 lanes per row
               _case(d + "_a5003", d, 3, 6, 5, 5003, (0, 2, 4)),                  # 64 lanes per row, unaligned rows
               _case(d + "_off", d, 3, 6, 5, 63, (1, 2), off=STORES[d][3])]       # element-wise gradient
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
