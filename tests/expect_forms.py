"""The kernel forms of libwarprnnt_expect.so (csrc/rnnt_expect.hip, rnnt_expect_f64.hip, rnnt_expect_h16.hip): which kernels
its three code objects hold, the release rule that picks them (a restatement of launch_ex_fwd / launch_ex_bwd,
csrc/rnnt_expect_impl.h) and the smallest cases that reach every form -- the counterpart of tests/bestpath_forms.py, with the
rectangles (`boundaries`) of tests/mi_forms.py.  tests/test_expect_cpu.py checks the table against the built code objects;
tests/test_gpu_expect.py runs every case with all outputs and checks that exactly the predicted kernels ran.

A case: dtype, N, S, T, mod (the modified type: px (N, S, T), the symbol edge consumes a frame).  The stages are "fwd" and
"bwd"; the host-scores entry adds "restore"."""
from tests import forms_common as C
from tests.forms_common import STORES, object_of                        # noqa: F401  (this table's names)
from tests.mi_forms import PATTERNS, boundaries                         # noqa: F401

OBJECTS = {"f32": "rnnt_expect.hip", "f64": "rnnt_expect_f64.hip", "h16": "rnnt_expect_h16.hip"}
STAGES = ("fwd", "bwd", "restore")
CHUNK = 4               # kExChunk: steps per prefetched chunk of the forward sweep (half of it for 8-byte storage)
CHUNK_BWD = 2           # kExChunkBwd: ... of the backward sweep (half of it for 8-byte storage)
WAVE_MAX_U = 64         # kExWaveMaxU: one wavefront up to here, on S + 1
BLOCK_MAX = 1024        # kExMaxU: a thread per row, the threads of a block


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"expect_fwd_kernel": "fwd", "expect_bwd_kernel": "bwd", "expect_restore_kernel": "restore"}.get(base)


def multi(case):
    return case["S"] + 1 > WAVE_MAX_U


def threads(case):
    return 64 if not multi(case) else (case["S"] + 1 + 63) // 64 * 64


def predict(case, cus=256, cost_grads=True, host=False):
    """{stage: set of kernel names} a call with all outputs launches for `case` (no rule depends on the compute units).
    Without gradient pointers: the fwd stage alone; cost_grads=False: cx_grad / cy_grad not taken; host: scalars in host
    memory."""
    tag = STORES[case["dtype"]][1]
    b = lambda v: "true" if v else "false"                                                   # noqa: E731
    out = {"fwd": {"rnnt::expect_fwd_kernel<%s, %s, %s>" % (tag, b(case["mod"]), b(multi(case)))},
           "bwd": {"rnnt::expect_bwd_kernel<%s, %s, %s, %s>" % (tag, b(case["mod"]), b(multi(case)), b(cost_grads))},
           "restore": set()}
    if host:
        out["restore"] = {"rnnt::expect_restore_kernel<%s>" % tag}
    return out


def steps(case):
    """Steps of a sweep over the full rectangle: anti-diagonals (regular) or frame columns (modified)."""
    return case["T"] + 1 if case["mod"] else case["T"] + case["S"] + 1


def _case(name, dtype, N, S, T, mod):
    assert S >= 0 and T >= 1 and (N >= PATTERNS or name.endswith("u1024"))
    return dict(name=name, dtype=dtype, N=N, S=S, T=T, mod=bool(mod))


def _cases():
    cs = []
    ty = ("reg", "mod")
    # every storage type, both types, both forms (S + 1 = 7, 65) and a full block (S + 1 = 1024); odd T: fp32 rows off the
    # 16-byte grid, T % 8 != 0: 16-bit rows off it
    for d in ("f32", "f64", "bf16", "f16"):
        for mod in (0, 1):
            cs += [_case("%s_%s_u7" % (d, ty[mod]), d, 7, 6, 9, mod),
                   _case("%s_%s_u65" % (d, ty[mod]), d, 7, 64, 70 if mod else 9, mod),
                   _case("%s_%s_u1024" % (d, ty[mod]), d, 2, 1023, 1025 if mod else 5, mod)]
    for d in ("f32", "f64"):
        for mod in (0, 1):
            n = "%s_%s" % (d, ty[mod])
            # the wave form: one row (px has no element), two rows, every lane live; the block form: three wavefronts
            cs += [_case(n + "_u1", d, 7, 0, 6, mod), _case(n + "_u2", d, 7, 1, 6, mod),
                   _case(n + "_u64", d, 7, 63, 66 if mod else 10, mod),
                   _case(n + "_u130", d, 7, 129, 140 if mod else 12, mod)]
            # steps of the sweeps around one chunk and three, at S = 3 (the regular type's shortest at S = 1: T >= 1)
            for st in (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1):
                S = 3 if mod or st - 4 >= 1 else 1
                cs.append(_case("%s_steps%d" % (n, st), d, 7, S, st - 1 if mod else st - S - 1, mod))
    # T around one and two wavefronts' worth of frames
    for i, T in enumerate((1, 2, 62, 63, 64, 65, 127, 128)):
        for mod in (0, 1):
            d = ("f32", "bf16", "f64", "f16")[(i + mod) % 4]
            cs.append(_case("%s_%s_t%d" % (d, ty[mod], T), d, 7, 5, T, mod))
    # the block form with longer rows, 16-bit storage
    cs += [_case("bf16_reg_s70_t67", "bf16", 7, 70, 67, 0), _case("f16_mod_s66_t97", "f16", 7, 66, 97, 1)]
    return cs


CASES = {c["name"]: c for c in _cases()}


def _other_forms():
    """(object, kernel) of the forms the one call with all outputs does not reach: no cost gradients; host scalars."""
    rows = set()
    for c in CASES.values():
        rows |= {(object_of(c), k) for k in predict(c, cost_grads=False)["bwd"]}
        rows |= {(object_of(c), k) for k in predict(c, host=True)["restore"]}
    return rows


# The kernels the one call with all outputs and device scalars never launches: the backward sweep without cost gradients and
# the restore of the host-scores entry.  tests/test_gpu_expect.py test_call_forms_agree runs them and checks their names.
UNREACHABLE = dict.fromkeys(_other_forms(), "reached by test_call_forms_agree, not by the one call with all outputs")


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rule reaches with CASES."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
