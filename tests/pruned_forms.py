"""The kernel forms of libwarprnnt_pruned.so (csrc/rnnt_pruned.hip, rnnt_pruned_f64.hip, rnnt_pruned_h16.hip): which kernels its
three code objects hold, the release rules that pick them (a restatement of run_pruned / run_prune_ranges, csrc/rnnt_pruned_impl.h,
and of launch_lattice / launch_coef, csrc/rnnt_host.h), and one case per form that reaches it -- the counterpart of
tests/kernel_forms.py and tests/joint_forms.py.  tests/test_pruned_cpu.py checks the table against the built code objects;
tests/test_gpu_pruned.py runs every case and checks that exactly the predicted kernels ran.

The prune-ranges entry runs the additive joint's partition stage unchanged (rnnt_joint_impl.h, launch_joint_partition): its forms
and the cases that reach them are joint_forms.py's, run through compute_rnnt_prune_ranges_add with S = 2.

A loss case: dtype, N, T, U (= maxU), A, S, entry "loss"; `off` = byte offset of the logits and gradients from a 16-byte
boundary (the element-wise gradient form).  A ranges case: the same with entry "ranges" (f, g instead of the logits)."""
from tests import forms_common as C
from tests import joint_forms as J
from tests import kernel_forms as K
from tests.forms_common import STORES, lattice_form, object_of, stats_group  # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_pruned.hip", "f64": "rnnt_pruned_f64.hip", "h16": "rnnt_pruned_h16.hip"}
JOINT_OBJECT = {"joint_f32": "f32", "joint_bf16": "h16", "joint_f16": "h16"}
STAGES = ("prep", "stats", "lattice", "coef", "grad", "partition", "window")
COEF_CELL_MAX_U = 48


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    if base in ("pruned_prep_kernel", "pruned_fix_kernel"):
        return "prep"
    if base == "pruned_stats_kernel":
        return "stats"
    if base.startswith("lattice"):
        return "lattice"
    if base.startswith("coef_"):
        return "coef"
    if base.startswith("pruned_grad"):
        return "grad"
    if base in ("pruned_window_kernel", "pruned_ranges_kernel"):
        return "window"
    if base.startswith("joint_"):
        return "partition"
    return None


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` on a device with `cus` compute units."""
    N, T, U, A = K.case_shape(case, cus)
    if case["entry"] == "ranges":
        jc = dict(case, entry="add")
        out = {s: set() for s in STAGES}
        out["partition"] = J.predict_joint(jc, cus)["partition"]
        out["lattice"] = {lattice_form("float", U, N, 2, cus)}
        out["window"] = {"rnnt::pruned_window_kernel<0>", "rnnt::pruned_ranges_kernel<0>"}
        return out
    obj, tag, lat, esz = STORES[case["dtype"]]
    off = case.get("off", 0)
    out = {s: set() for s in STAGES}
    out["prep"] = {"rnnt::pruned_prep_kernel<%s>" % lat, "rnnt::pruned_fix_kernel<%s>" % lat}
    out["stats"] = {"rnnt::pruned_stats_kernel<%s, %d>" % (tag, stats_group(A * esz))}
    out["lattice"] = {lattice_form(lat, U, N, 2, cus)}
    out["coef"] = {"rnnt::coef_kernel<%s, false>" % lat if U > COEF_CELL_MAX_U else "rnnt::coef_cell_kernel<%s>" % lat}
    out["grad"] = {"rnnt::pruned_grad_kernel<%s>" % tag if off % 16 == 0 else "rnnt::pruned_grad_elem_kernel<%s>" % tag}
    return out


def _case(name, dtype, N, T, U, A, S, entry="loss", **kw):
    return dict(name=name, dtype=dtype, N=N, T=T, U=U, A=A, S=S, entry=entry, **kw)


def _cases():
    # Shapes keep T (S - 1) >= maxU - 1, so that the full-length sample 0 has windows holding a path (a finite cost compared
    # with the reference) at every lattice width
    cs = []
    for d in ("f32", "f64", "bf16", "f16"):
        cs += [_case(d + "_a5", d, 4, 9, 7, 5, 3),                                  # 4 lanes per row, cell coefficients
               _case(d + "_a300", d, 3, 8, 6, 300, 2),                              # 16 lanes per row
               _case(d + "_a5003", d, 3, 5, 5, 5003, 4),                            # 64 lanes per row, unaligned rows
               _case(d + "_off", d, 3, 6, 5, 63, 2, off=STORES[d][3]),             # element-wise gradient
               _case(d + "_u65", d, 4, 8, 65, 7, 12),                               # lattice (8, 1), tiled coefficients
               _case(d + "_u300", d, 2, 5, 300, 3, 64),                             # lattice (4, 2)
               _case(d + "_u600", d, 2, 3, 600, 2, 300),                            # lattice (8, 2)
               _case(d + "_wide_n", d, "cus//2+1", 3, 9, 5, 4)]                     # past one block per CU: lattice (1, 1)
    # the joint's partition forms (joint_forms.FORMS rows of that stage), each through the ranges entry at S = 2
    seen = set()
    for obj, k, jname in J.FORMS:
        if J.jstage_of(k) != "partition" or (obj, jname) in seen:
            continue
        seen.add((obj, jname))
        jc = J.JCASES[jname]
        cs.append(_case("ranges_" + jname, jc["dtype"], jc["N"], jc["T"], max(jc["U"], 2), jc["A"], 2, entry="ranges",
                        off={"f": jc.get("off", {}).get("f", 0), "g": jc.get("off", {}).get("g", 0)}))
    return cs


CASES = {c["name"]: c for c in _cases()}

# Instantiations the build holds that no release rule of this library launches, with the reason (none: launch_coef's joint
# form, with coef_kernel<.., true>, is a template parameter this library never instantiates)
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def joint_unreachable():
    """Partition-stage instantiations the joint objects hold but no joint rule launches (joint_forms.UNREACHABLE)."""
    out = {}
    for jobj, ks in J.expected_inventory().items():
        for k, why in ks.items():
            if J.jstage_of(k) == "partition" and why.startswith("unreachable"):
                out[(JOINT_OBJECT[jobj], k)] = why
    return out


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), list(UNREACHABLE) + list(joint_unreachable()))
