"""The kernel forms of libwarprnnt_mi.so (csrc/rnnt_mi.hip, rnnt_mi_f64.hip, rnnt_mi_h16.hip): which kernels its three code
objects hold, the release rules that pick them (a restatement of run_mi / launch_mi_lattice, csrc/rnnt_mi_impl.h) and the
cases that reach every form -- the counterpart of tests/delay_forms.py.  tests/test_mi_cpu.py checks the table against the
built code objects; tests/test_gpu_mi.py runs every case with gradients and checks that exactly the predicted kernels ran.

A case: dtype, N, S, T, mod (the modified type: px (N, S, T), the symbol edge consumes a frame).  The rectangles come from
`boundaries(case, rng)`."""
import numpy as np

from tests import forms_common as C
from tests.forms_common import STORES, object_of                        # noqa: F401  (this table's names)

OBJECTS = {"f32": "rnnt_mi.hip", "f64": "rnnt_mi_f64.hip", "h16": "rnnt_mi_h16.hip"}
STAGES = ("pack", "lattice", "unpack")
CHUNK = 8               # kArChunk == kMonoChunk: diagonals / frames per chunk of the wave forms
WAVE_MAX_U = 64         # kArWaveMaxU == kMonoWaveMaxU: the release rule of the lattice, on S + 1
TILE = 32               # kMiTile: the transpose tile's edge
PATTERNS = 7            # rectangles of `boundaries`, by sample index modulo this


def stage_of(name):
    base = name.split("<")[0].split("::")[-1]
    return {"mi_pack_kernel": "pack", "ar_lattice_wave_kernel": "lattice", "ar_lattice_block_kernel": "lattice",
            "mono_lattice_wave_kernel": "lattice", "mono_lattice_block_kernel": "lattice", "mi_score_kernel": "lattice",
            "mi_unpack_kernel": "unpack"}.get(base)


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` with gradients (no rule depends on the compute-unit
    count).  A score-only call: the pack and lattice stages alone."""
    obj, tag, lat, esz = STORES[case["dtype"]]
    mod = "true" if case["mod"] else "false"
    form = "wave" if case["S"] + 1 <= WAVE_MAX_U else "block"
    return {"pack": {"rnnt::mi_pack_kernel<%s, %s>" % (tag, mod)},
            "lattice": {"rnnt::%s_lattice_%s_kernel<%s>" % ("mono" if case["mod"] else "ar", form, lat),
                        "rnnt::mi_score_kernel<%s>" % lat},
            "unpack": {"rnnt::mi_unpack_kernel<%s, %s>" % (tag, mod)}}


def boundaries(case, rng):
    """(N, 4) int64 rows [s0, t0, s1, t1].  By sample index modulo PATTERNS: 0 the full rectangle (the tensor's own
    dimensions are used), 1 t1 < T and s1 < S, 2 nonzero s0 / t0, 3 s1 == s0, 4 t1 == t0, 5 s1 - s0 == t1 - t0 (the modified
    type's single path), 6 s1 - s0 > t1 - t0 (the modified type: no path) -- each as far as S and T allow."""
    N, S, T = case["N"], case["S"], case["T"]
    bd = np.zeros((N, 4), np.int64)
    for b in range(N):
        k = b % PATTERNS
        s0, t0, s1, t1 = 0, 0, S, T
        if k == 1:
            s1 = int(rng.integers(0, S)) if S > 0 else 0
            t1 = int(rng.integers(1, T)) if T > 1 else 0
        elif k == 2:
            s0 = int(rng.integers(1, S + 1)) if S > 0 else 0
            t0 = int(rng.integers(1, max(T - 1, 1) + 1))
        elif k == 3:
            s0 = s1 = int(rng.integers(0, S + 1))
        elif k == 4:
            t0 = t1 = int(rng.integers(0, T + 1))
        elif k == 5:
            d = min(S, T)
            s0, t0 = S - d, T - d
        elif k == 6 and S > 0:
            t0 = T - min(S - 1, T)
        bd[b] = (s0, t0, s1, t1)
    return bd


def _case(name, dtype, N, S, T, mod):
    assert S >= 0 and T >= 1 and (N >= 5 or name.endswith("u1100"))
    return dict(name=name, dtype=dtype, N=N, S=S, T=T, mod=bool(mod))


def _cases():
    cs = []
    ty = ("reg", "mod")
    # every storage type, both types, both lattice forms (S + 1 = 7 and 65); the modified ones with room for S symbols
    for d in ("f32", "f64", "bf16", "f16"):
        for mod in (0, 1):
            cs += [_case("%s_%s_u7" % (d, ty[mod]), d, 7, 6, 9, mod),
                   _case("%s_%s_u65" % (d, ty[mod]), d, 7, 64, 70 if mod else 9, mod)]
    for d in ("f32", "f64"):
        for mod in (0, 1):
            n = "%s_%s" % (d, ty[mod])
            # the wave form: one column (px has no element), two columns, every lane live; the block form: more than two
            # wavefronts, and every thread of a full block with two columns
            cs += [_case(n + "_u1", d, 7, 0, 6, mod), _case(n + "_u2", d, 7, 1, 6, mod),
                   _case(n + "_u64", d, 7, 63, 66 if mod else 10, mod),
                   _case(n + "_u130", d, 7, 129, 140 if mod else 12, mod),
                   _case(n + "_u1100", d, 2, 1099, 1101 if mod else 5, mod)]
            # steps of the wave form's sweep around one chunk and three: the regular type walks (T + 1) + S diagonals of the
            # full rectangle, the modified type T frames
            for steps in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 3 * CHUNK, 3 * CHUNK + 1):
                cs.append(_case("%s_steps%d" % (n, steps), d, 7, 3, steps if mod else steps - 4, mod))
    # the transpose tile: S and T one below, at and one above its edge, on both axes.  The table is (T + 1 | T) x (S + 1) and
    # a row of px is T + 1 | T long beside py's T, so T = 31, 32 put the mismatch on a tile boundary in one type each
    for mod in (0, 1):
        for S in (TILE - 1, TILE, TILE + 1):
            for T in (TILE - 1, TILE, TILE + 1):
                d = "f64" if (S + T + mod) % 4 == 0 else "f32"
                cs.append(_case("%s_%s_s%d_t%d" % (d, ty[mod], S, T), d, 7, S, T, mod))
    # two tiles and a bit on both axes, 16-bit storage
    cs += [_case("bf16_reg_s70_t67", "bf16", 7, 70, 67, 0), _case("f16_mod_s66_t97", "f16", 7, 66, 97, 1)]
    return cs


CASES = {c["name"]: c for c in _cases()}
UNREACHABLE = {}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} the release rules reach with CASES on a device of `cus` compute units."""
    return C.predicted_rows(CASES, predict, cus)


def expected_inventory(cus=256):
    """{object: set of kernels} the three code objects must hold exactly."""
    return C.expected_inventory(OBJECTS, predicted_rows(cus), UNREACHABLE)
