"""The kernel forms of libwarprnnt_logprobs.so (csrc/rnnt_logprobs.hip, rnnt_logprobs_f64.hip, rnnt_logprobs_h16.hip): which
kernels its three code objects hold, the launch rule that picks them (a restatement of run_logprobs_fwd / run_logprobs_bwd,
csrc/rnnt_logprobs_impl.h) and, for each form the rule can pick, the smallest shapes that select it -- the counterpart of
tests/pstream_forms.py.  tests/test_logprobs_cpu.py checks the table against the built code objects;
tests/test_gpu_logprobs.py runs every case and checks that exactly the predicted kernels ran.

A case: dtype, K (0: the joint form; else the window width of the pruned form), mod (rnnt_type), B, T, U, C; `off` = byte offset
of the logits and their gradient from a 16-byte boundary (the element-wise backward by address, rows off the packet grid in
the forward)."""
import numpy as np

from tests import forms_common as FC
from tests.forms_common import STORES, object_of                        # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_logprobs.hip", "f64": "rnnt_logprobs_f64.hip", "h16": "rnnt_logprobs_h16.hip"}
STAGES = ("lse", "edges", "grad")
NARROW_BYTES, WIDE_BYTES = 256, 2048                    # kLpNarrowBytes, kLpWideBytes
TILE = 256                                              # the block of logprobs_edges_kernel along the outputs' t-fastest order


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"logprobs_lse_kernel": "lse", "logprobs_edges_kernel": "edges", "logprobs_grad_kernel": "grad"}.get(base)


def lanes(case):
    """lp_lanes: the lanes of a row in the forward."""
    row = case["C"] * STORES[case["dtype"]][3]
    return FC.stats_group(row, WIDE_BYTES, NARROW_BYTES)


def vec(case):
    return case.get("off", 0) % 16 == 0 and (case["C"] * STORES[case["dtype"]][3]) % 16 == 0


def predict(case, cus=256):
    """{stage: set of kernel names} a forward and a backward call launch for `case` (no rule depends on the compute units)."""
    tag = STORES[case["dtype"]][1]
    return {"lse": {"rnnt::logprobs_lse_kernel<%s, %d>" % (tag, lanes(case))},
            "edges": {"rnnt::logprobs_edges_kernel<%s>" % tag},
            "grad": {"rnnt::logprobs_grad_kernel<%s, %s>" % (tag, "true" if vec(case) else "false")}}


def boundary(case, rng):
    """int64 (B, 4) rows [0, 0, S_b, T_b]: sample 0 full; then, as far as B reaches, one without a frame, one without a symbol;
    the rest random."""
    B, T, S = case["B"], case["T"], case["U"] - 1
    sb = rng.integers(0, S + 1, size=B)
    tb = rng.integers(1, T + 1, size=B)
    sb[0], tb[0] = S, T
    if B > 1:
        tb[1] = 0
    if B > 2:
        sb[2] = 0
    return np.stack([np.zeros(B, int), np.zeros(B, int), sb, tb], 1).astype(np.int64)


def ranges(case, rng):
    """(B, T) int32 starts in [0, U - K]: frame 0 at 0, the last frame at U - K, between them NOT monotone in t."""
    B, T, U, K = case["B"], case["T"], case["U"], case["K"]
    out = rng.integers(0, U - K + 1, size=(B, T)).astype(np.int32)
    out[:, 0] = 0
    out[:, -1] = U - K
    return out


def _case(name, dtype, K, mod, B, T, U, C, **kw):
    assert 0 <= K <= U and mod in (0, 1)
    return dict(name=name, dtype=dtype, K=K, mod=mod, B=B, T=T, U=U, C=C, **kw)


def _cases():
    cs = []
    for i, d in enumerate(("f32", "f64", "bf16", "f16")):
        esz = STORES[d][3]
        pk = 16 // esz
        form = lambda k: (0, 2)[(i + k) % 2]                             # noqa: E731  joint / pruned at K = 2
        mod = lambda k: ((i + k) // 2) % 2                               # noqa: E731
        cs += [
            # the four forms at the smallest packet row: 4 lanes, 16-byte packets in the backward
            _case(d + "_joint_regular", d, 0, 0, 3, 4, 3, 2 * pk),
            _case(d + "_joint_modified", d, 0, 1, 3, 4, 3, 2 * pk),
            _case(d + "_pruned_regular", d, 2, 0, 3, 4, 4, 2 * pk),
            _case(d + "_pruned_modified", d, 2, 1, 3, 4, 4, 2 * pk),
            # rows off the packet grid (odd C: 16-bit rows are not even 4-byte aligned) and bases off the boundary
            _case(d + "_odd", d, form(0), mod(0), 3, 4, 3, 7),
            _case(d + "_off", d, form(1), mod(1), 3, 4, 3, 2 * pk, off=esz),
            _case(d + "_odd_off", d, form(0), mod(1), 2, 3, 3, 2 * pk + 1, off=esz),
            # both sides of the two row-length thresholds of the forward
            _case(d + "_narrow_last", d, form(1), mod(0), 2, 3, 3, NARROW_BYTES // esz),
            _case(d + "_mid_first", d, form(0), mod(1), 2, 3, 3, NARROW_BYTES // esz + 1),
            _case(d + "_mid_first_vec", d, form(1), mod(0), 2, 3, 3, NARROW_BYTES // esz + pk),
            _case(d + "_mid_last", d, form(0), mod(0), 2, 3, 3, WIDE_BYTES // esz),
            _case(d + "_wide_first", d, form(1), mod(1), 2, 3, 3, WIDE_BYTES // esz + 1),
            _case(d + "_wide_first_vec", d, form(0), mod(1), 2, 3, 3, WIDE_BYTES // esz + pk),
            # more packets than one round of 64 lanes x 4 (and C > 4096), more than 256 accesses per row in the backward
            _case(d + "_c4100", d, form(1), mod(0), 2, 2, 3, 4100 if esz != 2 else 4104),
            _case(d + "_c4099", d, form(0), mod(1), 1, 2, 2, 4099),
        ]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the launch rule reaches with CASES."""
    return FC.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return FC.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
