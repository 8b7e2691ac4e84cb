"""The kernel forms of libwarprnnt_hat.so (csrc/rnnt_hat.hip, rnnt_hat_f64.hip, rnnt_hat_h16.hip): which kernels its three code
objects hold, the release rules that pick them (a restatement of run_hat / launch_hat_stats /
launch_hat_grad, csrc/rnnt_hat_impl.h, and of launch_lattice / launch_coef, csrc/rnnt_host.h), and one case per form that
reaches it -- the counterpart of tests/tdt_forms.py.  tests/test_hat_cpu.py checks the table against the built code objects;
tests/test_gpu_hat.py runs every case and checks that exactly the predicted kernels ran.

A case: dtype, N, T, U (= maxU), A, blank; `off` = byte offset of the logits and gradients from a 16-byte boundary (the
element-wise gradient form).  The blank sits at column 0, at A - 1 and at interior columns that are not the first lane of a
16-byte packet."""
from tests import forms_common as C
from tests.forms_common import STORES, lattice_form, object_of          # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_hat.hip", "f64": "rnnt_hat_f64.hip", "h16": "rnnt_hat_h16.hip"}
STAGES = ("stats", "lattice", "coef", "grad")


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"hat_stats_kernel": "stats", "lattice_kernel": "lattice", "lattice_lin_kernel": "lattice",
            "coef_kernel": "coef", "coef_cell_kernel": "coef", "hat_grad_kernel": "grad",
            "hat_grad_elem_kernel": "grad"}.get(base)


WIDE_ROW_BYTES = 4096   # kHatWideRowBytes: rows up to here stay on 16 lanes


def stats_group(row_bytes):
    """launch_hat_stats: stats_grid with HAT's threshold."""
    return C.stats_group(row_bytes, WIDE_ROW_BYTES)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` on a device of `cus` compute units (a training
    call: both lattice directions)."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    N, U = case["N"], case["U"]
    lattice = lattice_form(lat, U, N, 2, cus)
    coef = "rnnt::coef_cell_kernel<%s>" % lat if U <= 48 else "rnnt::coef_kernel<%s, false>" % lat
    grad = "rnnt::hat_grad_kernel<%s>" % tag if case.get("off", 0) % 16 == 0 else "rnnt::hat_grad_elem_kernel<%s>" % tag
    return {"stats": {"rnnt::hat_stats_kernel<%s, %d>" % (tag, stats_group(case["A"] * esz))},
            "lattice": {lattice}, "coef": {coef}, "grad": {grad}}


def _case(name, dtype, N, T, U, A, blank, **kw):
    return dict(name=name, dtype=dtype, N=N, T=T, U=U, A=A, blank=blank, **kw)


def _cases():
    cs = []
    for d in ("f32", "f64", "bf16", "f16"):
        cs += [_case(d + "_a5", d, 4, 9, 7, 5, 2),                        # 4 lanes per row; linear lattice (fp64: <1, 1>)
               _case(d + "_a300", d, 3, 8, 6, 300, 299),                   # 16 lanes per row, blank last
               _case(d + "_a1025", d, 3, 8, 6, 1025, 0),                   # 16 lanes per row, unaligned 2 KB+ rows, blank first
               _case(d + "_a5003", d, 3, 6, 5, 5003, 2501),                # 64 lanes per row, unaligned rows, blank interior
               _case(d + "_off", d, 3, 6, 5, 63, 17, off=STORES[d][3]),    # element-wise gradient
               _case(d + "_lat81", d, 3, 30, 100, 6, 5),                   # lattice <8, 1>, tiled coefficients
               _case(d + "_lat42", d, 3, 12, 300, 5, 3),                   # lattice <4, 2>
               _case(d + "_lat82", d, 3, 10, 600, 5, 1)]                   # lattice <8, 2>
        if d != "f64":
            cs.append(_case(d + "_lat11", d, 300, 6, 5, 5, 1))             # more blocks than compute units: lattice <1, 1>
        # the blank in column 0 and in column A - 1, each time in a packet shared with the neighbouring row, at every group
        # size: 256-byte rows one element off the boundary (17 packets: a second round at 4 lanes), rows just past 256 and
        # just past 4096 bytes (257 packets or more: a second round at 64 lanes)
        esz = STORES[d][3]
        for g, A, kw in ((4, 256 // esz, dict(off=esz)), (16, 256 // esz + 1, {}), (64, WIDE_ROW_BYTES // esz + 1, {})):
            cs += [_case("%s_g%d_b0" % (d, g), d, 3, 4, 3, A, 0, **kw), _case("%s_g%d_blast" % (d, g), d, 3, 4, 3, A, A - 1, **kw)]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
