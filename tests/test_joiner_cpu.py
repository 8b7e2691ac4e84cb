"""No GPU: the fp64 reference of the fused joiner (tests/joiner_ref.py) against torch autograd of the three torch routes it
replaces -- act(f[:, :, None] + g[:, None]), pack_joint of that, and act(am_p + lm_p) of prune_inputs; libwarprnnt_joiner.so's
C-ABI, export map and code objects against include/rnnt_joiner.h and tests/joiner_forms.py; the build lists; the argument program
under the host sanitizers; and the refusals of warprnnt_pytorch.joiner that need no device."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import joiner_forms as F
from tests import joiner_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_joiner.so", "rnnt_joiner.h"
TORCH_ACT = {"identity": lambda x: x, "relu": torch.relu, "tanh": torch.tanh}


def _problem(seed, N=3, T=5, U=4, H=3, S=2):
    rng = np.random.default_rng(seed)
    f, g = rng.standard_normal((N, T, H)), rng.standard_normal((N, U, H))
    tl, ll = np.array([T, 1, 3][:N]), np.array([U - 1, 0, 2][:N])
    ranges = F.ranges(dict(N=N, T=T, U=U, S=S), rng)
    return rng, f, g, tl, ll, ranges


def _torch_route(layout, name, f, g, tl, ll, ranges, S, dout):
    """(out, df, dg) of the torch route of a layout, fp64 on the CPU; the padding of the padded tensor and of its gradient is
    zero, as the definition's."""
    from warprnnt_pytorch.packed import pack_joint
    from warprnnt_pytorch.pruned import prune_inputs
    ft, gt = torch.tensor(f, requires_grad=True), torch.tensor(g, requires_grad=True)
    if layout == R.PRUNED:
        am_p, lm_p = prune_inputs(ft, gt, torch.tensor(ranges), S)
        out = TORCH_ACT[name](am_p + lm_p)
        if tl is not None:
            out = out * (torch.arange(f.shape[1])[None, :] < torch.tensor(tl)[:, None])[:, :, None, None]
    else:
        out = TORCH_ACT[name](ft[:, :, None] + gt[:, None])
        if layout == R.PACKED:
            out = pack_joint(out, torch.tensor(tl), torch.tensor(ll))
        elif tl is not None:
            mask = ((torch.arange(f.shape[1])[None, :, None] < torch.tensor(tl)[:, None, None])
                    & (torch.arange(g.shape[1])[None, None, :] <= torch.tensor(ll)[:, None, None]))
            out = out * mask[..., None]
    out.backward(torch.tensor(dout))
    return out.detach().numpy(), ft.grad.numpy(), gt.grad.numpy()


@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("layout,lens", [(0, True), (0, False), (1, True), (2, True), (2, False)])
@pytest.mark.parametrize("seed", range(3))
def test_reference_equals_torch_autograd(seed, layout, lens, name):
    rng, f, g, tl, ll, ranges = _problem(seed)
    N, T, U, S = 3, 5, 4, 2
    if not lens:
        tl = ll = None
    out = R.forward(f, g, layout, name, tl, ll, ranges, S)
    dout = rng.standard_normal(out.shape)
    df, dg, af, ag, nf, ng = R.backward(out, dout, layout, name, N, T, U, tl, ll, ranges, S)
    tout, tdf, tdg = _torch_route(layout, name, f, g, tl, ll, ranges, S, dout)
    assert np.abs(out - tout).max() <= 1e-12 and np.abs(df - tdf).max() <= 1e-12 and np.abs(dg - tdg).max() <= 1e-12
    # the sums of |e| bound the sums, and the counts are those of the layout
    assert (np.abs(df) <= af + 1e-15).all() and (np.abs(dg) <= ag + 1e-15).all()
    rows = R.rows(layout, N, T, U, tl, ll, ranges, S)
    assert nf.sum() == ng.sum() == len(rows) and out.shape == R.out_shape(layout, N, T, U, 3, tl, ll, S)
    if layout == 2:
        assert (nf[nf > 0] == S).all()
    mask = R.real_mask(layout, out.shape, N, T, U, tl, ll, ranges, S)
    assert not out[~mask].any() and mask.sum() == len(rows)


def test_reference_bad_start_zeroes_the_sample():
    rng, f, g, tl, ll, ranges = _problem(7)
    ranges[1, 0], ranges[2, 4] = -1, 4                      # sample 1: a read frame; sample 2: frame 4 >= T_2 = 3, not read
    out = R.forward(f, g, 2, "tanh", tl, None, ranges, 2)
    assert list(R.bad_samples(ranges, tl, 4)) == [False, True, False]
    assert not out[1].any() and out[0].any() and out[2, :3].any() and not out[2, 3:].any()
    df, dg, *_ = R.backward(out, np.ones_like(out), 2, "tanh", 3, 5, 4, tl, None, ranges, 2)
    assert not df[1].any() and not dg[1].any() and df[0].any()
    ranges[1, 0] = 4                                        # U itself
    assert list(R.bad_samples(ranges, np.array([5, 5, 5]), 4)) == [False, True, True]


def test_jumping_starts_leave_label_rows_without_gradient():
    f, g = np.ones((1, 3, 2)), np.ones((1, 9, 2))
    ranges = np.array([[0, 4, 8]], np.int32)
    out = R.forward(f, g, 2, "identity", None, None, ranges, 2)
    _, dg, _, _, _, ng = R.backward(out, np.ones_like(out), 2, "identity", 1, 3, 9, None, None, ranges, 2)
    assert list(ng[0]) == [1, 1, 0, 0, 1, 1, 0, 0, 2] and not dg[0, 2].any() and (dg[0, 8] == 2).all()


# ----------------------------------------------------------------------------- the table
def test_the_table_names_every_form_and_threshold():
    cs = F.CASES.values()
    for d in ("f32", "f64", "bf16", "f16"):
        mine = [c for c in cs if c["dtype"] == d]
        for layout in (0, 1, 2):
            assert {F.plan(c)["vec"] for c in mine if c["layout"] == layout} == {True, False}
        plans = [(c, F.plan(c)) for c in mine]
        assert any(p["single"] and p["TZ"] > 1 and p["vec"] for _, p in plans) and any(p["single"] and p["TZ"] > 1 and not p["vec"] for _, p in plans)
        assert any(p["single"] and p["lds"] == F.LDS_BYTES and p["threads"] == 64 and p["vec"] for _, p in plans)
        assert any(p["single"] and p["lds"] == F.LDS_BYTES and not p["vec"] for _, p in plans)
        assert any(not p["single"] and p["vec"] for _, p in plans) and any(not p["single"] and not p["vec"] for _, p in plans)
        assert any(p["single"] and p["slices"] > 1 and p["Pb"] % p["CX"] for _, p in plans)
        assert any(c["layout"] == 2 and not p["single"] for c, p in plans) and any(c.get("full") for c in mine)
        assert all(p["lds"] <= F.LDS_BYTES and p["CX"] * p["TY"] <= 256 for _, p in plans if p["single"])
        assert any(c.get("off") for c in mine)
    assert {c["act"] for c in cs} == set(R.ACTS)
    split = F.CASES["f32_split"]
    assert (split["T"], split["U"], split["N"], split["H"]) == (130, 3, 1, 8) and F.plan(split)["TZ"] == 8
    assert F.shares(128, 150, 512) == 1 and F.shares(16, 375, 512) == 8 and F.shares(64, 375, 512) == 2


def test_the_tables_constants_are_the_drivers():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_joiner_impl.h")).read()
    assert "constexpr size_t kJnLdsBytes = 64 * 1024;" in text and F.LDS_BYTES == 64 * 1024
    assert "constexpr int kJnBlocks = %d;" % F.BLOCKS in text and "constexpr int kJnMaxShares = %d;" % F.MAX_SHARES in text


def test_the_ranges_generator():
    for name, c in F.CASES.items():
        if c["layout"] == 2:
            r = F.ranges(c, np.random.default_rng(1))
            assert r.shape == (c["N"], c["T"]) and r.dtype == np.int32 and r.min() >= 0 and r.max() == c["U"] - 1, name
    r = F.ranges(F.CASES["f32_pruned_u65"], np.random.default_rng(1))
    assert (np.diff(r[0]) > 3).any()                        # a jump of more than S: label rows without a window


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header_and_the_map():
    declared = I.declared(HEADER)
    assert declared == {"get_workspace_size_joiner", "compute_rnnt_joiner_fwd", "compute_rnnt_joiner_bwd"}
    text = open(os.path.join(ROOT, "warp-transducer_amd", "exports_joiner.map")).read()
    assert set(re.findall(r"^\s+(\w+);", text, re.M)) == declared
    assert I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any("joiner" in s for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import joiner
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(joiner.EXPORTS, HEADER) == []
    # the backward call is the forward's with (out, dout, df, dg) in the place of (f, g, out)
    assert sigs["compute_rnnt_joiner_bwd"] == ["pointer"] + sigs["compute_rnnt_joiner_fwd"]
    assert sigs["get_workspace_size_joiner"] == ["int"] * 7 + ["size_t*"]


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for tag in ("F32", "F64", "BF16", "F16"):
        for v in ("true", "false"):
            for kernel in ("fwd", "bwd", "df", "dg"):
                assert "rnnt::joiner_%s_kernel<rnnt::%s, %s>" % (kernel, tag, v) in ks
        assert "rnnt::joiner_prep_kernel<rnnt::%s>" % tag in ks and "rnnt::joiner_dg_sum_kernel<rnnt::%s>" % tag in ks


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
    mk = os.path.join("warp-transducer_amd", "Makefile")
    for path, pattern in (("setup.py", '("joiner",)'), (mk, "SIDE += pstream\nSIDE += joiner\n"),
                          (mk, "build/asan/test_joiner_args"), (mk, "$(filter-out joiner,$(SIDE_ARGS))"),
                          ("CMakeLists.txt", "list(APPEND SIDE_LIBS joiner)"), ("MANIFEST.in", "exports_joiner.map")):
        assert pattern in open(os.path.join(ROOT, path)).read(), (path, pattern)
    for unit in F.OBJECTS.values():
        assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "csrc", unit))
    assert os.path.exists(os.path.join(ROOT, "warp-transducer_amd", "cabi_tests", "test_joiner_args.cpp"))


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_joiner_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_joiner_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_joiner_args" in mk
    assert "build/asan/test_joiner_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def test_importing_the_package_does_not_load_the_library():
    code = ("import sys\nsys.path.insert(0, %r)\nimport warprnnt_pytorch\nfrom warprnnt_pytorch import joiner\n"
            "assert joiner._LIB._handle is None\n"
            "assert not any('libwarprnnt_joiner' in line for line in open('/proc/self/maps'))\n"
            "assert not hasattr(warprnnt_pytorch, 'joiner_padded')\nprint('ok')\n" % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr[-3000:]


def test_a_missing_library_is_an_import_error(tmp_path):
    code = ("import sys\nsys.path.insert(0, %r)\nfrom warprnnt_pytorch import joiner\n"
            "try:\n    joiner.lib()\nexcept ImportError as e:\n    print(e)\nelse:\n    sys.exit('loaded something')\n"
            % os.path.join(ROOT, "warp-transducer_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WARP_RNNT_PATH=str(tmp_path)), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.strip() == ("libwarprnnt_joiner.so not found at %s -- build it with `make -C warp-transducer_amd`. "
                                  "There is no fallback for the fused joiner." % (tmp_path / "libwarprnnt_joiner.so"))


def test_python_refusals_that_need_no_device():
    from warprnnt_pytorch import joiner
    f, g = torch.zeros(2, 3, 4), torch.zeros(2, 2, 4)
    i32 = dict(dtype=torch.int32)
    tl, ll, rg = torch.tensor([3, 2], **i32), torch.tensor([1, 0], **i32), torch.zeros(2, 3, **i32)
    calls = {"padded": lambda: joiner.joiner_padded(f, g, tl, ll), "packed": lambda: joiner.joiner_packed(f, g, tl, ll),
             "pruned": lambda: joiner.joiner_pruned(f, g, rg, 2, tl),
             "module": lambda: joiner.TransducerJoint()(f, g, tl, ll + 1),
             "module packed": lambda: joiner.TransducerJoint("tanh", pack_output=True)(f, g, tl, ll + 1)}
    for name, fn in calls.items():
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == "the fused joiner runs on the GPU only: f is on cpu, g is on cpu", name
    for bad in ("gelu", "Tanh", "", None, 2):
        with pytest.raises(ValueError, match="'identity', 'relu' or 'tanh'"):
            joiner.joiner_padded(f, g, activation=bad)
        with pytest.raises(ValueError, match="'identity', 'relu' or 'tanh'"):
            joiner.TransducerJoint(activation=bad)
    with pytest.raises(ValueError, match="must be a 3D tensor"):
        joiner.joiner_padded(f[0], g)
    with pytest.raises(ValueError, match="needs act_lens and label_lens"):
        joiner.joiner_packed(f, g, None, ll)
    m = joiner.TransducerJoint("tanh", pack_output=True, validate=False)
    assert (m.activation, m.pack_output, m.validate) == ("tanh", True, False)
    assert [joiner.act_code(a) for a in R.ACTS] == [0, 1, 2] and (joiner.PADDED, joiner.PACKED, joiner.PRUNED) == (0, 1, 2)
