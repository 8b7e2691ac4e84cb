"""The kernel forms of libwarprnnt_bestpath.so (csrc/rnnt_bestpath.hip, rnnt_bestpath_f64.hip, rnnt_bestpath_h16.hip): which
kernels its three code objects hold, the release rule that picks them (a restatement of launch_bp_sweep / launch_bp_edges,
csrc/rnnt_bestpath_impl.h) and the smallest cases that reach every form -- the counterpart of tests/mi_forms.py, whose
rectangles (`boundaries`) the cases use.  tests/test_bestpath_cpu.py checks the table against the built code objects;
tests/test_gpu_bestpath.py runs every case with all outputs and checks that exactly the predicted kernels ran.

A case: dtype, N, S, T, mod (the modified type: px (N, S, T), the symbol edge consumes a frame).  The sweep and the traceback
share ONE launch (bestpath_sweep_kernel: the block that swept a sample walks it back), so the stages are "sweep" -- both --
and "edges"."""
from tests import forms_common as C
from tests.forms_common import STORES, object_of                        # noqa: F401  (this table's names)
from tests.mi_forms import PATTERNS, boundaries                         # noqa: F401

OBJECTS = {"f32": "rnnt_bestpath.hip", "f64": "rnnt_bestpath_f64.hip", "h16": "rnnt_bestpath_h16.hip"}
STAGES = ("sweep", "edges")
CHUNK = 8               # kBpChunk: steps per prefetched chunk, a row per thread
CHUNK_WIDE = 2          # kBpChunkWide: ... with WIDE_ROWS rows per thread
WIDE_ROWS = 4           # kBpWideRows
WAVE_MAX_U = 64         # kBpWaveMaxU: one wavefront up to here, on S + 1
BLOCK_MAX = 1024        # threads of a block: above it WIDE_ROWS rows per thread
LDS_WORDS = 6144        # kBpLdsWords: the traceback's staging
TILE = 256              # the block of bestpath_edges_kernel along t


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"bestpath_sweep_kernel": "sweep", "bestpath_edges_kernel": "edges"}.get(base)


def form(case):
    """(K, MULTI) of the sweep."""
    U = case["S"] + 1
    return (1, False) if U <= WAVE_MAX_U else (1, True) if U <= BLOCK_MAX else (WIDE_ROWS, True)


def threads(case):
    K, multi = form(case)
    return 64 if not multi else (-(-(case["S"] + 1) // K) + 63) // 64 * 64


def predict(case, cus=256):
    """{stage: set of kernel names} a call with all outputs launches for `case` (no rule depends on the compute units).
    Without px_path / py_path: the sweep stage alone; compute_rnnt_bestpath_edges: the edges stage alone."""
    tag = STORES[case["dtype"]][1]
    mod = "true" if case["mod"] else "false"
    K, multi = form(case)
    return {"sweep": {"rnnt::bestpath_sweep_kernel<%s, %s, %d, %s>" % (tag, mod, K, "true" if multi else "false")},
            "edges": {"rnnt::bestpath_edges_kernel<%s, %s>" % (tag, mod)}}


def steps(case):
    """Steps of the sweep over the full rectangle: anti-diagonals (regular) or frame columns (modified)."""
    return case["T"] + 1 if case["mod"] else case["T"] + case["S"] + 1


def _case(name, dtype, N, S, T, mod):
    assert S >= 0 and T >= 1 and (N >= PATTERNS or name.endswith("u1100"))
    return dict(name=name, dtype=dtype, N=N, S=S, T=T, mod=bool(mod))


def _cases():
    cs = []
    ty = ("reg", "mod")
    # every storage type, both types, the three forms (S + 1 = 7, 65 and 1100); odd T: fp32 rows off the 16-byte
    # grid, T % 8 != 0: 16-bit rows off it
    for d in ("f32", "f64", "bf16", "f16"):
        for mod in (0, 1):
            cs += [_case("%s_%s_u7" % (d, ty[mod]), d, 7, 6, 9, mod),
                   _case("%s_%s_u65" % (d, ty[mod]), d, 7, 64, 70 if mod else 9, mod),
                   _case("%s_%s_u1100" % (d, ty[mod]), d, 2, 1099, 1101 if mod else 5, mod)]
    for d in ("f32", "f64"):
        for mod in (0, 1):
            n = "%s_%s" % (d, ty[mod])
            # the wave form: one row (px has no element), two rows, every lane live; the block form: three wavefronts
            cs += [_case(n + "_u1", d, 7, 0, 6, mod), _case(n + "_u2", d, 7, 1, 6, mod),
                   _case(n + "_u64", d, 7, 63, 66 if mod else 10, mod),
                   _case(n + "_u130", d, 7, 129, 140 if mod else 12, mod)]
            # steps of the sweep around one chunk and three
            for st in (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1):
                cs.append(_case("%s_steps%d" % (n, st), d, 7, 3, st - 1 if mod else st - 4, mod))
    # the 64-bit word boundary of back: T + 1 nodes per row
    for i, T in enumerate((62, 63, 64, 65, 127, 128)):
        for mod in (0, 1):
            d = ("f32", "bf16", "f64", "f16")[(i + mod) % 4]
            cs.append(_case("%s_%s_t%d" % (d, ty[mod], T), d, 7, 5, T, mod))
    # the block form across a word boundary, 16-bit storage
    cs += [_case("bf16_reg_s70_t67", "bf16", 7, 70, 67, 0), _case("f16_mod_s66_t97", "f16", 7, 66, 97, 1)]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rule reaches with CASES."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
