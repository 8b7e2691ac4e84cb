"""No GPU: the fp64 reference of the lattice primitive on px / py (tests/mi_ref.py) against brute-force path enumeration
and closed forms; libwarprnnt_mi.so's C-ABI and code objects against include/rnnt_mi.h and tests/mi_forms.py; the build
lists; and the refusals of warprnnt_pytorch.mi that need no device."""
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import mi_forms as F
from tests import mi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_mi.so", "rnnt_mi.h"
NEG = float("-inf")


def _random(rng, B, S, T, mod, holes=0.0):
    px = rng.standard_normal((B, S, T if mod else T + 1)) - 1.0
    py = rng.standard_normal((B, S + 1, T)) - 1.0
    if holes:
        px[rng.random(px.shape) < holes] = NEG
        py[rng.random(py.shape) < holes] = NEG
    return px, py


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("seed", range(24))
def test_reference_equals_brute_force(seed):
    """Scores of tiny rectangles, -inf edges included, against the enumeration of their paths; the occupations against
    central differences of the enumeration."""
    rng = np.random.default_rng(4000 + seed)
    mod = seed % 2 == 1
    B, S, T = 3, int(rng.integers(0, 4)), int(rng.integers(1, 5))
    px, py = _random(rng, B, S, T, mod, holes=0.2 if seed % 3 == 0 else 0.0)
    bd = F.boundaries(dict(N=B, S=S, T=T), rng)
    bd[0] = (0, 0, S, T)
    w = rng.random(B) + 0.5
    sc, gx, gy = R.mi_autograd(px, py, bd, w)

    def brute(px_, py_, b):
        s0, t0, s1, t1 = bd[b]
        return R.mi_brute(px_[b, s0:s1, t0:(t1 if mod else t1 + 1)], py_[b, s0:s1 + 1, t0:t1], mod)

    mx, my = R.edge_masks(B, S, T, mod, bd)
    assert not gx[~mx].any() and not gy[~my].any()
    for b in range(B):
        want = brute(px, py, b)
        assert (sc[b] == want) if want == NEG else abs(sc[b] - want) < 1e-12, (b, sc[b], want)
        if want == NEG:
            assert not gx[b].any() and not gy[b].any()
            continue
        assert (gx[b] >= -1e-12).all() and (gx[b] <= w[b] + 1e-12).all()
        h = 1e-6
        for arr, g in ((px, gx), (py, gy)):
            for idx in zip(*np.nonzero(np.isfinite(arr[b]) & (mx if arr is px else my)[b])):
                hi, lo = arr.copy(), arr.copy()
                hi[(b,) + idx] += h
                lo[(b,) + idx] -= h
                a = (hi, py) if arr is px else (px, hi)
                z = (lo, py) if arr is px else (px, lo)
                fd = (brute(*a, b) - brute(*z, b)) / (2 * h) * w[b]
                assert abs(fd - g[(b,) + idx]) < 1e-6, (b, idx, fd, g[(b,) + idx])


@pytest.mark.parametrize("mod", [False, True])
def test_closed_form_single_path(mod):
    """Regular, t1 == t0: the symbols are emitted at one frame position, score = sum_s px[s, t0].  Modified, s1 - s0 ==
    t1 - t0: every frame carries a symbol, score = sum of the diagonal of px.  Every edge of the path has occupation 1."""
    rng = np.random.default_rng(1)
    S, T = 4, 6
    px, py = _random(rng, 1, S, T, mod)
    if mod:
        bd = np.array([[0, 2, 4, 6]], np.int64)
        want = sum(px[0, i, 2 + i] for i in range(4))
    else:
        bd = np.array([[0, 3, 4, 3]], np.int64)
        want = px[0, :, 3].sum()
    sc, gx, gy = R.mi_autograd(px, py, bd)
    assert abs(sc[0] - want) < 1e-12
    assert abs(gx.sum() - 4) < 1e-12 and set(np.round(gx[gx != 0], 12)) == {1.0} and not gy.any()


@pytest.mark.parametrize("mod", [False, True])
def test_closed_form_without_symbols(mod):
    """S = 0: one path along the frames, score = sum_t py[0, t0 .. t1 - 1]; px has no element."""
    rng = np.random.default_rng(2)
    px, py = _random(rng, 2, 0, 7, mod)
    bd = np.array([[0, 0, 0, 7], [0, 2, 0, 5]], np.int64)
    sc, gx, gy = R.mi_autograd(px, py, bd)
    assert gx.size == 0 and abs(sc[0] - py[0, 0].sum()) < 1e-12 and abs(sc[1] - py[1, 0, 2:5].sum()) < 1e-12
    assert np.array_equal(gy[1, 0], np.array([0, 0, 1, 1, 1, 0, 0], np.float64))


@pytest.mark.parametrize("mod", [False, True])
def test_closed_form_uniform_lattice(mod):
    """Every edge at weight w: the score is the log of the number of paths plus the weight of one -- C(S + T, S) paths of
    S + T edges (regular), C(T, S) paths of T edges (modified; none when S > T)."""
    for S, T, w in ((3, 5, -0.7), (5, 5, 0.3), (6, 4, -1.1), (0, 3, -2.0)):
        px = np.full((1, S, T if mod else T + 1), w)
        py = np.full((1, S + 1, T), w)
        sc, gx, gy = R.mi_autograd(px, py)
        if mod:
            want = math.log(math.comb(T, S)) + T * w if S <= T else NEG
        else:
            want = math.log(math.comb(S + T, S)) + (S + T) * w
        assert sc[0] == want if want == NEG else abs(sc[0] - want) < 1e-12, (S, T, sc, want)
        if want != NEG:                                    # a path has S symbol edges and T (regular) or T - S frame edges
            assert abs(gx.sum() - S) < 1e-10 and abs(gy.sum() - (T - S if mod else T)) < 1e-10


def test_the_tables_generators():
    for name, case in F.CASES.items():
        bd = F.boundaries(case, np.random.default_rng(1))
        N, S, T = case["N"], case["S"], case["T"]
        assert bd.shape == (N, 4) and bd.dtype == np.int64 and tuple(bd[0]) == (0, 0, S, T), name
        assert (0 <= bd[:, 0]).all() and (bd[:, 0] <= bd[:, 2]).all() and (bd[:, 2] <= S).all(), name
        assert (0 <= bd[:, 1]).all() and (bd[:, 1] <= bd[:, 3]).all() and (bd[:, 3] <= T).all(), name
        if N >= F.PATTERNS:
            assert bd[3, 0] == bd[3, 2] and bd[4, 1] == bd[4, 3], name
            assert bd[5, 2] - bd[5, 0] == bd[5, 3] - bd[5, 1], name
            assert S == 0 or bd[6, 2] - bd[6, 0] > bd[6, 3] - bd[6, 1], name
            if S > 1 and T > 2:
                assert bd[1, 2] < S and bd[1, 3] < T and bd[2, 0] > 0 and bd[2, 1] > 0, name
    # the full modified rectangles have a path, but for the tile cases with S > T
    for name, case in F.CASES.items():
        assert not case["mod"] or case["S"] <= case["T"] or "_s" in name, name


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_exports_map_names_the_header():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_mi.map")).read()
    for name in I.declared(HEADER):
        assert "    %s;\n" % name in text
    assert text.count(";") == len(I.declared(HEADER)) + 2          # the four names, `*;` and the closing brace


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in ("libwarprnnt.so", "libwarprnnt_ar.so", "libwarprnnt_mono.so", "libwarprnnt_delay.so"):
        got = I.exports(os.path.join(I.LIBDIR, lib))
        assert got and not any(s.endswith("_mi") or "_mi_" in s for s in got), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import mi
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(mi.EXPORTS, HEADER) == []


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for tag in ("F32", "F64", "BF16", "F16"):
        for mod in ("true", "false"):
            for stage in ("pack", "unpack"):
                assert "rnnt::mi_%s_kernel<rnnt::%s, %s>" % (stage, tag, mod) in ks
    for obj, lat in (("f32", "float"), ("f64", "double"), ("h16", "float")):
        assert (obj, "rnnt::mi_score_kernel<%s>" % lat) in rows
        for lattice in ("ar", "mono"):
            for form in ("wave", "block"):
                assert (obj, "rnnt::%s_lattice_%s_kernel<%s>" % (lattice, form, lat)) in rows
    for mod in (False, True):
        cs = [c for c in F.CASES.values() if c["mod"] == mod]
        assert {c["S"] + 1 for c in cs} >= {1, 2, F.WAVE_MAX_U, F.WAVE_MAX_U + 1, 130, 1100}
        steps = {c["T"] if mod else c["T"] + 1 + c["S"] for c in cs if c["S"] + 1 <= F.WAVE_MAX_U}
        assert steps >= {F.CHUNK - 1, F.CHUNK, F.CHUNK + 1, 3 * F.CHUNK, 3 * F.CHUNK + 1}
        edge = {F.TILE - 1, F.TILE, F.TILE + 1}
        assert {(c["S"], c["T"]) for c in cs} >= {(s, t) for s in edge for t in edge}
    assert all(c["N"] >= 5 for n, c in F.CASES.items() if not n.endswith("u1100"))


def test_the_tables_constants_are_the_kernels():
    csrc = os.path.join(ROOT, "warp-transducer_amd", "csrc")
    text = open(os.path.join(csrc, "rnnt_ar_kernels.h")).read()
    assert "constexpr int kArChunk = %d;" % F.CHUNK in text and "constexpr int kArWaveMaxU = %d;" % F.WAVE_MAX_U in text
    text = open(os.path.join(csrc, "rnnt_mono_kernels.h")).read()
    assert "constexpr int kMonoChunk = %d;" % F.CHUNK in text and "constexpr int kMonoWaveMaxU = %d;" % F.WAVE_MAX_U in text
    assert "constexpr int kMiTile = %d;" % F.TILE in open(os.path.join(csrc, "rnnt_mi_kernels.h")).read()


def test_device_code_has_no_scratch():
    """No scratch, no spilled VGPRs (tools/check_kernel_resources.py) in any of the three code objects."""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as res
    import check_lattice_lin_isa as guard
    for unit in F.OBJECTS.values():
        asm = guard.device_asm(None, os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
        assert res.kernels(asm) and res.check(asm) == [], unit


def test_build_lists_name_the_library():
    for path, pattern in (("setup.py", '"mi"'), (os.path.join("warp-transducer_amd", "Makefile"), "SIDE += mi\n"),
                          (os.path.join("warp-transducer_amd", "Makefile"), "build/asan/test_mi_args"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS mi)"), ("MANIFEST.in", "exports_mi.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), path
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_mi_args.cpp"))


# ----------------------------------------------------------------------------- the Python module, without a device
def test_python_refuses_cpu_tensors_and_bad_shapes():
    """Shapes, dtypes, contiguity and the boundary's description are checked before the device, so all of them can be seen
    here; a CPU tensor that passes them is refused as such, whatever `validate` says."""
    from warprnnt_pytorch.mi import mutual_information_recursion as mir
    px, py = torch.zeros(2, 3, 6), torch.zeros(2, 4, 5)
    for kw in ({}, dict(return_grad=True), dict(validate=False), dict(boundary=torch.zeros(2, 4, dtype=torch.int64))):
        with pytest.raises(ValueError, match="GPU only"):
            mir(px, py, **kw)
    with pytest.raises(ValueError, match="GPU only"):
        mir(torch.zeros(2, 3, 5), py)                                  # the modified type
    with pytest.raises(ValueError, match="3D"):
        mir(px[0], py)
    for bad in (torch.zeros(2, 3, 7), torch.zeros(2, 3, 4), torch.zeros(2, 4, 6), torch.zeros(3, 3, 6)):
        with pytest.raises(ValueError, match=r"px must be \(B, S, T \+ 1\) or \(B, S, T\)"):
            mir(bad, py)
    with pytest.raises(ValueError, match="one dtype"):
        mir(px.double(), py)
    with pytest.raises(ValueError, match="one dtype"):
        mir(px.long(), py.long())
    with pytest.raises(ValueError, match="contiguous"):
        mir(torch.zeros(2, 6, 3).transpose(1, 2), py)
    with pytest.raises(ValueError, match="T >= 1"):
        mir(torch.zeros(2, 3, 0), torch.zeros(2, 4, 0))
    for bad in (torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int64),
                [[0, 0, 3, 5]] * 2):
        with pytest.raises(ValueError, match=r"int64 tensor of shape \(B, 4\)"):
            mir(px, py, boundary=bad)
    with pytest.raises(ValueError, match="boundary must be contiguous"):
        mir(px, py, boundary=torch.zeros(4, 2, dtype=torch.int64).t())
    import warprnnt_pytorch
    assert not hasattr(warprnnt_pytorch, "mutual_information_recursion")    # a submodule: the package exports no side module
