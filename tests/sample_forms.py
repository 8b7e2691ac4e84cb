"""The kernel forms of libwarprnnt_sample.so (csrc/rnnt_sample.hip, rnnt_sample_f64.hip, rnnt_sample_h16.hip): which kernels
its three code objects hold, the release rule that picks them (a restatement of run_sample_type, csrc/rnnt_sample_impl.h) and
the smallest cases that reach every form -- tests/expect_forms.py's table with the number of walks K added, on the
rectangles (`boundaries`) of tests/mi_forms.py.  tests/test_sample_cpu.py checks the table against the built code objects and
every case's seed against the decision margin; tests/test_gpu_sample.py runs every case and checks that exactly the
predicted kernels ran.

A case: dtype, N, S, T, mod (the modified type: px (N, S, T), the symbol edge consumes a frame), K, seed (of its uniforms).
The stages are "fwd" and "walk" (entry 1), "weights" (entry 3) and "edges" (entry 4)."""
import zlib

import numpy as np

from tests import forms_common as C
from tests.forms_common import STORES, object_of                        # noqa: F401  (this table's names)
from tests.mi_forms import PATTERNS, boundaries                         # noqa: F401

OBJECTS = {"f32": "rnnt_sample.hip", "f64": "rnnt_sample_f64.hip", "h16": "rnnt_sample_h16.hip"}
STAGES = ("fwd", "walk", "weights", "edges")
CHUNK = 8               # kSaChunk: steps per prefetched chunk of the sweep (half of it for 8-byte storage)
WAVE_MAX_U = 64         # kSaWaveMaxU: one wavefront up to here, on S + 1
BLOCK_MAX = 1024        # kSaMaxU: a thread per row, the threads of a block
MAX_K = 1024            # kSaMaxK
WALK_BLOCK = 256        # kSaWalkBlock
KS = (1, 3, 64, 65, 130)
# cases whose default seed (0) left a decision inside the margin: tests/test_sample_cpu.py test_every_decision_is_clear
SEEDS = {}


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"sample_fwd_kernel": "fwd", "sample_walk_kernel": "walk", "path_weights_kernel": "weights",
            "path_edges_kernel": "edges"}.get(base)


def multi(case):
    return case["S"] + 1 > WAVE_MAX_U


def threads(case):
    return 64 if not multi(case) else (case["S"] + 1 + 63) // 64 * 64


def walk_block(K):
    return WALK_BLOCK if K >= WALK_BLOCK else (K + 63) // 64 * 64


def chunk(case):
    return CHUNK // 2 if case["dtype"] == "f64" else CHUNK


def predict(case, cus=256, entries=(1, 3, 4)):
    """{stage: set of kernel names} the entries `entries` launch for `case` (no rule depends on the compute units).  Entry 2:
    the walk stage alone."""
    tag = STORES[case["dtype"]][1]
    b = lambda v: "true" if v else "false"                                                   # noqa: E731
    out = {s: set() for s in STAGES}
    if 1 in entries:
        out["fwd"] = {"rnnt::sample_fwd_kernel<%s, %s, %s>" % (tag, b(case["mod"]), b(multi(case)))}
    if 1 in entries or 2 in entries:
        out["walk"] = {"rnnt::sample_walk_kernel<%s, %s>" % (tag, b(case["mod"]))}
    if 3 in entries:
        out["weights"] = {"rnnt::path_weights_kernel<%s, %s>" % (tag, b(case["mod"]))}
    if 4 in entries:
        out["edges"] = {"rnnt::path_edges_kernel<%s, %s>" % (tag, b(case["mod"]))}
    return out


def steps(case):
    """Steps of a sweep over the full rectangle: anti-diagonals (regular) or frame columns (modified)."""
    return case["T"] + 1 if case["mod"] else case["T"] + case["S"] + 1


def uniforms(case):
    """(N, K, S + T) float32 in [0, 1) of the case's seed."""
    rng = np.random.default_rng([zlib.crc32(case["name"].encode()), case["seed"]])
    return rng.random((case["N"], case["K"], case["S"] + case["T"]), dtype=np.float32)


def problem(case):
    """px, py of the case's storage type (torch, on the CPU): weights around -1.5, NaN outside every rectangle's edge sets;
    the boundary rows, the two edge masks and the uniforms.  The CPU test judges the seeds on exactly these values."""
    import torch
    from tests.mi_ref import edge_masks
    dt = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}[case["dtype"]]
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    bd = boundaries(case, rng)
    N, S, T, mod = case["N"], case["S"], case["T"], case["mod"]
    px = torch.tensor(rng.standard_normal((N, S, T if mod else T + 1)) - 1.5, dtype=torch.float32).to(dt)
    py = torch.tensor(rng.standard_normal((N, S + 1, T)) - 1.5, dtype=torch.float32).to(dt)
    mx, my = edge_masks(N, S, T, mod, bd)
    px[torch.tensor(~mx)] = float("nan")
    py[torch.tensor(~my)] = float("nan")
    return px, py, bd, mx, my, uniforms(case)


_count = [0]


def _case(name, dtype, N, S, T, mod, K=None):
    assert S >= 0 and T >= 1 and (N >= PATTERNS or name.endswith("u1024"))
    if K is None:
        K = KS[_count[0] % len(KS)]
        _count[0] += 1
    return dict(name=name, dtype=dtype, N=N, S=S, T=T, mod=bool(mod), K=K, seed=SEEDS.get(name, 0))


def _cases():
    cs = []
    ty = ("reg", "mod")
    # every storage type, both types, both forms (S + 1 = 7, 65) and a full block (S + 1 = 1024, few walks: the reference
    # pays for each); odd T: fp32 rows off the 16-byte grid, T % 8 != 0: 16-bit rows off it
    for i, d in enumerate(("f32", "f64", "bf16", "f16")):
        for mod in (0, 1):
            cs += [_case("%s_%s_u7" % (d, ty[mod]), d, 7, 6, 9, mod),
                   _case("%s_%s_u65" % (d, ty[mod]), d, 7, 64, 70 if mod else 9, mod),
                   _case("%s_%s_u1024" % (d, ty[mod]), d, 2, 1023, 1025 if mod else 5, mod, K=(1, 3)[(i + mod) % 2])]
    for d in ("f32", "f64"):
        for mod in (0, 1):
            n = "%s_%s" % (d, ty[mod])
            # the wave form: one row (px has no element), two rows, every lane live; the block form: three wavefronts
            cs += [_case(n + "_u1", d, 7, 0, 6, mod), _case(n + "_u2", d, 7, 1, 6, mod),
                   _case(n + "_u64", d, 7, 63, 66 if mod else 10, mod),
                   _case(n + "_u130", d, 7, 129, 140 if mod else 12, mod)]
            # steps of the sweep around one chunk and three, at S = 3 (the regular type's shortest at S = 1: T >= 1)
            ch = CHUNK // 2 if d == "f64" else CHUNK
            for st in (ch - 1, ch, ch + 1, 3 * ch - 1, 3 * ch, 3 * ch + 1):
                S = 3 if mod or st - 4 >= 1 else 1
                cs.append(_case("%s_steps%d" % (n, st), d, 7, S, st - 1 if mod else st - S - 1, mod))
    # T around one wavefront's worth of frames
    for i, T in enumerate((1, 2, 63, 64, 65)):
        for mod in (0, 1):
            d = ("f32", "bf16", "f64", "f16")[(i + mod) % 4]
            cs.append(_case("%s_%s_t%d" % (d, ty[mod], T), d, 7, 5, T, mod))
    # every K with both types (the walk's block is 64, 128 or 192 threads), fp32 and 16-bit storage
    for K in KS:
        for mod in (0, 1):
            d = ("f32", "f16", "bf16")[(K + mod) % 3]
            cs.append(_case("%s_%s_k%d" % (d, ty[mod], K), d, 7, 8, 19 if mod else 11, mod, K=K))
    return cs


CASES = {c["name"]: c for c in _cases()}

# Entry 1 with entries 3 and 4 behind it reaches every kernel of the library.
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rule reaches with CASES."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
