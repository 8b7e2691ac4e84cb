"""The kernel forms of libwarprnnt_joiner.so (csrc/rnnt_joiner.hip, rnnt_joiner_f64.hip, rnnt_joiner_h16.hip): which kernels its
three code objects hold, the launch rule that picks them (a restatement of jn_plan / jn_shares, csrc/rnnt_joiner_impl.h) and,
for each form the rule can pick, the smallest shapes that select it -- the counterpart of tests/pstream_forms.py.
tests/test_joiner_cpu.py checks the table against the built code objects; tests/test_gpu_joiner.py runs every case and checks
that exactly the predicted kernels ran.

A case: dtype, layout (0 padded, 1 packed, 2 pruned), act, N, T, U, S (layout 2), H; `off` = byte offset of every tensor of the
calls from a 16-byte boundary (the element-wise forms by address); `full`: no lengths are passed (layouts 0 and 2)."""
import numpy as np

from tests import forms_common as C
from tests.forms_common import STORES, object_of                        # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_joiner.hip", "f64": "rnnt_joiner_f64.hip", "h16": "rnnt_joiner_h16.hip"}
STAGES = ("prep", "fwd", "bwd", "sum", "df", "dg")
LDS_BYTES, BLOCKS, MAX_SHARES = 64 * 1024, 1024, 8         # kJnLdsBytes, kJnBlocks, kJnMaxShares


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"joiner_prep_kernel": "prep", "joiner_fwd_kernel": "fwd", "joiner_bwd_kernel": "bwd", "joiner_dg_sum_kernel": "sum",
            "joiner_df_kernel": "df", "joiner_dg_kernel": "dg"}.get(base)


def shares(N, T, H):
    """jn_shares: the workgroups of the single pass along T."""
    base = N * ((H + 63) // 64)
    return max(1, min(-(-BLOCKS // base), min(MAX_SHARES, (T + 15) // 16)))


def plan(case):
    """jn_plan: (vec, single, threads, CX, TY, TZ, lds bytes) of the backward call; vec is the forward's too."""
    esz = STORES[case["dtype"]][3]
    comp = 8 if case["dtype"] == "f64" else 4
    vec = case.get("off", 0) % 16 == 0 and (case["H"] * esz) % 16 == 0
    vb = (2 if esz == 8 else 4) if vec else 1
    fit = LDS_BYTES // (case["U"] * vb * comp)
    threads = 0 if fit < 1 else 1 << (min(fit, 256).bit_length() - 1)
    single = threads >= 64 and case["N"] <= 65535
    pb = case["H"] // vb
    cx = min(16, 1 << max(pb - 1, 0).bit_length())
    return dict(vec=vec, single=single, threads=threads, CX=cx, TY=threads // cx if single else 1,
                TZ=shares(case["N"], case["T"], case["H"]) if single else 1, lds=case["U"] * threads * vb * comp,
                slices=-(-pb // cx), Pb=pb)


def predict(case, cus=256):
    """{stage: set of kernel names} a forward and a backward call launch for `case` (no rule depends on the compute units)."""
    tag = STORES[case["dtype"]][1]
    p = plan(case)
    v = "true" if p["vec"] else "false"
    want = {"fwd": {"rnnt::joiner_fwd_kernel<%s, %s>" % (tag, v)}}
    if case["layout"] == 2:
        want["prep"] = {"rnnt::joiner_prep_kernel<%s>" % tag}
    if p["single"]:
        want["bwd"] = {"rnnt::joiner_bwd_kernel<%s, %s>" % (tag, v)}
        if p["TZ"] > 1:
            want["sum"] = {"rnnt::joiner_dg_sum_kernel<%s>" % tag}
    else:
        want["df"] = {"rnnt::joiner_df_kernel<%s, %s>" % (tag, v)}
        want["dg"] = {"rnnt::joiner_dg_kernel<%s, %s>" % (tag, v)}
    return want


def lengths(case, rng):
    """(T_b, L_b): sample 0 full; then, as far as N reaches, one sample with one frame and one without a label; the rest random."""
    N, T, U = case["N"], case["T"], case["U"]
    tl = rng.integers(1, T + 1, size=N)
    ll = rng.integers(0, U, size=N)
    tl[0], ll[0] = T, U - 1
    if N > 1:
        tl[1] = 1
    if N > 2:
        ll[2] = 0
    return tl.astype(np.int32), ll.astype(np.int32)


def ranges(case, rng):
    """(N, T) int32 window starts in [0, U - 1]: non-decreasing, with jumps of more than S (label rows no window covers) and a
    tail that runs into the clamp (start + k > U - 1)."""
    N, T, U, S = case["N"], case["T"], case["U"], case["S"]
    out = np.zeros((N, T), np.int32)
    for b in range(N):
        steps = rng.integers(0, S + 2, size=T)
        steps[0] = 0
        out[b] = np.minimum(np.cumsum(steps), U - 1)
        out[b, -1] = U - 1                                     # S > 1: the whole window but its first slot is clamped
    return out


def _case(name, dtype, layout, act, N, T, U, H, S=0, **kw):
    assert layout in (0, 1, 2) and act in ("identity", "relu", "tanh") and (layout != 2 or 1 <= S <= U)
    return dict(name=name, dtype=dtype, layout=layout, act=act, N=N, T=T, U=U, H=H, S=S, **kw)


def _cases():
    cs = []
    acts = ("identity", "relu", "tanh")
    for i, d in enumerate(("f32", "f64", "bf16", "f16")):
        esz = STORES[d][3]
        a = lambda k: acts[(i + k) % 3]                                  # noqa: E731
        lay = lambda k: (i + k) % 3                                      # noqa: E731
        elem_last = LDS_BYTES // (64 * (8 if d == "f64" else 4))        # the last U of the element-wise single pass: 256 (128)
        # forward, per layout: 16-byte packets and element-wise (H * esz off the packet, the address off the boundary)
        for layout in (0, 1, 2):
            S = 2 if layout == 2 else 0
            cs += [_case("%s_l%d_vec" % (d, layout), d, layout, a(layout), 3, 5, 4, 16 // esz * 2, S),
                   _case("%s_l%d_elem" % (d, layout), d, layout, a(layout + 1), 3, 5, 4, 7, S),
                   _case("%s_l%d_off" % (d, layout), d, layout, a(layout + 2), 3, 5, 4, 16 // esz * 2, S, off=esz)]
        cs += [
            # more frames than one workgroup's frame groups hold, one sample: the walk split over T (8 shares of 17 frames)
            _case(d + "_split", d, lay(0), a(0), 1, 130, 3, 8, 2 if lay(0) == 2 else 0),
            _case(d + "_split_elem", d, lay(1), a(1), 2, 40, 3, 5, 2 if lay(1) == 2 else 0),
            # several column slices, the last one partial (H = 520: 130 accumulator groups of 4 fp32, 16 to a slice)
            _case(d + "_h520", d, lay(2), a(2), 1, 5, 4, 520, 3 if lay(2) == 2 else 0),
            # the LDS accumulators: the last U of the single pass (64 threads, all of the 64 KiB) and the first of the fallback
            _case(d + "_u64", d, lay(0), a(1), 1, 3, 64, 8, 3 if lay(0) == 2 else 0),
            _case(d + "_u65", d, lay(1), a(2), 1, 3, 65, 8, 3 if lay(1) == 2 else 0),
            _case(d + "_elem_last", d, lay(2), a(0), 1, 3, elem_last, 3, 3 if lay(2) == 2 else 0),
            _case(d + "_elem_first", d, lay(0), a(2), 1, 3, elem_last + 1, 3, 3 if lay(0) == 2 else 0),
            _case(d + "_u600", d, lay(1), a(0), 1, 3, 600, 8, 3 if lay(1) == 2 else 0),
            # the fallback on windows: label rows without a window, and the clamped duplicates on row U - 1
            _case(d + "_pruned_u65", d, 2, a(1), 2, 6, 65, 8, 3),
            _case(d + "_pruned_u65_full", d, 2, a(2), 2, 6, 65, 8, 3, full=True),
            _case(d + "_padded_full", d, 0, a(0), 2, 5, 4, 8, full=True),
        ]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the launch rule reaches with CASES."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
