"""The kernel forms of libwarprnnt_kd.so (csrc/rnnt_kd.hip, rnnt_kd_f64.hip, rnnt_kd_h16.hip): which kernels its three code
objects hold, the release rules that pick them (a restatement of run_kd / launch_kd_stats / launch_kd_grad,
csrc/rnnt_kd_impl.h), and one case per form that reaches it -- the counterpart of tests/hat_forms.py.  tests/test_kd_cpu.py
checks the table against the built code objects; tests/test_gpu_kd.py runs every case and checks that exactly the predicted
kernels ran.

A case: dtype, mode (0 collapsed, 1 full), N, T, U (= maxU), A, blank; `off` = byte offset of the student logits, the teacher
logits and the gradients from a 16-byte boundary (the element-wise gradient form), `toff` = the same of the teacher alone (the
two rows of the statistics kernel then start at different offsets inside their first packets; the full mode's gradient
reads the teacher and goes element by element, the collapsed mode's does not and stays with the packet stream).

The statistics rule: 4 lanes per row up to 256 bytes, 16 up to 2048 bytes, 64 beyond; the t* cases sit on both sides of
each threshold."""
from tests import forms_common as C
from tests.forms_common import STORES, object_of, stats_group  # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_kd.hip", "f64": "rnnt_kd_f64.hip", "h16": "rnnt_kd_h16.hip"}
STAGES = ("stats", "cost", "grad")
MODES = ("collapsed", "full")


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"kd_stats_kernel": "stats", "kd_cost_kernel": "cost", "kd_grad_kernel": "grad",
            "kd_grad_elem_kernel": "grad"}.get(base)


def predict(case, cus=256):
    """{stage: set of kernel names} the release rules launch for `case` (a training call)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    mode = case["mode"]
    aligned = case.get("off", 0) % 16 == 0 and (mode == 0 or case.get("toff", 0) % 16 == 0)
    grad = "rnnt::kd_grad_kernel<%s, %d>" % (tag, mode) if aligned else "rnnt::kd_grad_elem_kernel<%s, %d>" % (tag, mode)
    return {"stats": {"rnnt::kd_stats_kernel<%s, %d, %d>" % (tag, stats_group(case["A"] * esz), mode)},
            "cost": {"rnnt::kd_cost_kernel<%s>" % lat}, "grad": {grad}}


def _case(name, dtype, mode, N, T, U, A, blank, **kw):
    return dict(name=name, dtype=dtype, mode=mode, N=N, T=T, U=U, A=A, blank=blank, **kw)


def _cases():
    cs = []
    for d in ("f32", "f64", "bf16", "f16"):
        esz = STORES[d][3]
        for m in (0, 1):
            p = "%s_%s_" % (d, MODES[m])
            cs += [_case(p + "a5", d, m, 4, 9, 7, 5, 2),                     # 4 lanes per row, rows shorter than two packets
                   _case(p + "a300", d, m, 3, 8, 6, 300, 299),               # 16 lanes (fp64: 64), blank last
                   _case(p + "a1025", d, m, 3, 8, 6, 1025, 0),               # 64 lanes, unaligned rows, blank first
                   _case(p + "a5003", d, m, 3, 6, 5, 5003, 2501),            # 64 lanes, several rounds, blank interior
                   _case(p + "off", d, m, 3, 6, 5, 63, 17, off=esz)]         # element-wise gradient (fp64: 16 lanes)
            if d in ("f32", "bf16"):
                cs += [_case(p + "a2", d, m, 4, 5, 4, 2, 1),                 # A = 2: the rest class is empty
                       _case(p + "a3", d, m, 4, 5, 4, 3, 0),                 # rows shorter than a packet
                       _case(p + "toff", d, m, 3, 6, 5, 63, 17, toff=esz),   # the teacher alone off its boundary
                       _case(p + "t256", d, m, 2, 3, 3, 256 // esz, 5),      # 4 lanes at the threshold ...
                       _case(p + "t256p", d, m, 2, 3, 3, 256 // esz + 1, 5),  # ... 16 one element past it
                       _case(p + "t2048", d, m, 2, 3, 3, 2048 // esz, 5),    # 16 lanes at the threshold ...
                       _case(p + "t2048p", d, m, 2, 3, 3, 2048 // esz + 1, 5)]   # ... 64 one element past it
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
