"""No GPU: the distillation loss's fp64 reference (tests/kd_ref.py) -- the gradient formula of include/rnnt_kd.h against
autograd over the header's edge cases, closed forms, kd_loss_torch against the reference; libwarprnnt_kd.so's C-ABI and code
objects against include/rnnt_kd.h and tests/kd_forms.py; the Python module's argument errors; _side.forward's unchanged
default; and the argument checks of the library under the sanitizers (make side-asan's test_kd_args)."""
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import inventory as I
from tests import kd_forms as F
from tests import kd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB, HEADER = "libwarprnnt_kd.so", "rnnt_kd.h"


def _tiny(seed, A=None, N=3):
    rng = np.random.default_rng(7000 + seed)
    T, U = int(rng.integers(1, 6)), int(rng.integers(1, 5))
    A = A or int(rng.integers(2, 9))
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    ll[1] = 0                                                     # L_b = 0
    blank = (0, A - 1, A // 2)[seed % 3]                          # first / last / interior
    z = rng.standard_normal((N, T, U, A)) * 2
    w = rng.standard_normal((N, T, U, A)) * 2
    labels = rng.integers(-2, A + 2, size=(N, max(U - 1, 1))).astype(np.int32)[:, :U - 1]     # some out of range: clamped
    if U > 1:
        labels[0, 0] = blank                                      # a label equal to the blank: a row of two classes
    return z, w, labels, tl, ll, blank, rng


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tau", [0.5, 2.0])
@pytest.mark.parametrize("seed", range(12))
def test_gradient_formula_of_the_header(seed, tau, mode):
    z, w, labels, tl, ll, blank, rng = _tiny(seed)
    wts = rng.random(len(tl)) + 0.5
    c, g = R.kd_autograd(z, w, labels, tl, ll, blank, mode, tau, wts)
    f = R.kd_formula(z, w, labels, tl, ll, blank, mode, tau) * wts[:, None, None, None]
    mask = R.in_lattice_mask(z.shape, tl, ll)
    assert (c > -1e-12).all() and np.allclose(g, f, rtol=1e-12, atol=1e-14)
    assert not g[~mask].any() and g[mask].any()


@pytest.mark.parametrize("A", [2, 3, 7, 50])
def test_formula_at_the_alphabets_of_the_issue(A):
    """A = 2 (the rest class is empty beside a label), 3, 7, 50; label == blank, no label, tau = 0.5 and 2."""
    for tau in (0.5, 2.0):
        for mode in (0, 1):
            z, w, labels, tl, ll, blank, _ = _tiny(A, A=A)
            _, g = R.kd_autograd(z, w, labels, tl, ll, blank, mode, tau)
            assert np.abs(g - R.kd_formula(z, w, labels, tl, ll, blank, mode, tau)).max() < 1e-14


def test_closed_forms():
    """One row: the collapsed loss of a row with two classes is the KL of two Bernoullis; the full loss the KL of the two
    softmaxes; teacher == student costs 0 with a zero gradient; the collapsed loss never exceeds the full one."""
    rng = np.random.default_rng(1)
    A, blank, tau = 6, 2, 1.5
    z, w = rng.standard_normal((1, 1, 1, A)), rng.standard_normal((1, 1, 1, A))
    nolab = np.zeros((1, 0), np.int32)
    p = np.exp(z / tau) / np.exp(z / tau).sum()
    q = np.exp(w / tau) / np.exp(w / tau).sum()
    pb, qb = p[..., blank].item(), q[..., blank].item()
    c0, _ = R.kd_autograd(z, w, nolab, [1], [0], blank, 0, tau)
    c1, _ = R.kd_autograd(z, w, nolab, [1], [0], blank, 1, tau)
    assert abs(c0[0] - (qb * np.log(qb / pb) + (1 - qb) * np.log((1 - qb) / (1 - pb)))) < 1e-13
    assert abs(c1[0] - (q * np.log(q / p)).sum()) < 1e-13 and c0[0] <= c1[0]
    for mode in (0, 1):
        c, g = R.kd_autograd(z, z, nolab, [1], [0], blank, mode, tau)
        assert abs(c[0]) < 1e-15 and np.abs(g).max() < 1e-15


def test_modes_and_operands_differ():
    """What the GPU test's negative controls rely on: the collapsed and the full loss, and the loss with student and teacher
    swapped, are different numbers."""
    z, w, labels, tl, ll, blank, _ = _tiny(4, A=7)
    c0, _ = R.kd_autograd(z, w, labels, tl, ll, blank, 0)
    c1, _ = R.kd_autograd(z, w, labels, tl, ll, blank, 1)
    cs, _ = R.kd_autograd(w, z, labels, tl, ll, blank, 0)
    assert np.abs(c0 - c1).min() > 1e-3 and np.abs(c0 - cs).min() > 1e-3


def test_cost_mag_bounds_the_cost():
    z, w, labels, tl, ll, blank, _ = _tiny(5, A=40)
    for mode in (0, 1):
        c, _ = R.kd_autograd(z, w, labels, tl, ll, blank, mode)
        assert (R.cost_mag(z, w, labels, tl, ll, blank, mode) >= c - 1e-12).all()


def test_rows_reference_equals_the_lattice_reference():
    z, w, labels, tl, ll, blank, _ = _tiny(6, A=9)
    N, T, U, A = z.shape
    lab = R.class_labels(labels, ll, blank, A, U)
    c, g = R.kd_autograd(z, w, labels, tl, ll, blank, 0, 2.0)
    rows = [(b, t, u) for b in range(N) for t in range(tl[b]) for u in range(ll[b] + 1)]
    kl, gr, cm, gm = R.kd_rows(np.stack([z[r] for r in rows]), np.stack([w[r] for r in rows]),
                               np.array([lab[b, u] for b, _, u in rows]), blank, 2.0)
    for b in range(N):
        assert abs(sum(k for k, r in zip(kl, rows) if r[0] == b) - c[b]) < 1e-12
    assert np.allclose(gr, np.stack([g[r] for r in rows]), atol=1e-14) and (cm > 0).all() and (gm >= np.abs(gr) - 1e-15).all()


@pytest.mark.parametrize("mode", ["collapsed", "full"])
@pytest.mark.parametrize("seed", range(6))
def test_kd_loss_torch_equals_the_reference(seed, mode):
    """The plain-torch route of warprnnt_pytorch.kd, on CPU tensors in fp64, NaN in its padding rows."""
    from warprnnt_pytorch.kd import kd_loss_torch
    z, w, labels, tl, ll, blank, rng = _tiny(seed)
    mask = R.in_lattice_mask(z.shape, tl, ll)
    tau = (0.5, 2.0)[seed % 2]
    wts = rng.random(len(tl)) + 0.5
    c, g = R.kd_autograd(z, w, labels, tl, ll, blank, F.MODES.index(mode), tau, wts)
    zn, wn = z.copy(), w.copy()
    zn[~mask] = np.nan
    wn[~mask] = np.nan
    zt = torch.tensor(zn, requires_grad=True)
    teacher = torch.tensor(wn, requires_grad=True)
    got = kd_loss_torch(zt, teacher, torch.tensor(labels), torch.tensor(tl), torch.tensor(ll), blank, mode, tau, "none")
    (got * torch.tensor(wts)).sum().backward()
    assert np.allclose(got.detach().numpy(), c, rtol=1e-12, atol=1e-13)
    assert np.allclose(zt.grad.numpy(), g, rtol=1e-11, atol=1e-13) and teacher.grad is None
    for red, want in (("sum", c.sum()), ("mean", c.mean())):
        r = kd_loss_torch(zt, teacher, torch.tensor(labels), torch.tensor(tl), torch.tensor(ll), blank, mode, tau, red)
        assert r.shape == (1,) and abs(r.item() - want) < 1e-12 * max(1.0, abs(want))


# ----------------------------------------------------------------------------- the built library
def test_exports_equal_the_header():
    declared = I.declared(HEADER)
    assert len(declared) == 4 and I.exports(I.need_lib(LIB)) == declared


def test_other_libraries_export_nothing_of_this_one():
    I.need_lib(LIB)
    for lib in sorted(os.listdir(I.LIBDIR)):
        if lib.endswith(".so") and lib != LIB:
            assert not any("_kd" in s for s in I.exports(os.path.join(I.LIBDIR, lib))), lib


def test_python_bindings_match_the_header():
    from warprnnt_pytorch import kd
    sigs = I.declared_signatures(HEADER)
    assert set(sigs) == I.declared(HEADER) and all(sigs.values())
    assert I.binding_faults(kd.EXPORTS, HEADER) == []
    # HAT's parameter lists with the teacher right behind the activations and (mode, temperature) behind the dtype code
    hat = I.declared_signatures("rnnt_hat.h")
    assert sigs["get_workspace_size_kd"] == hat["get_workspace_size_hat"]
    for name in ("compute_kd_loss", "compute_kd_loss_fwd", "compute_kd_loss_bwd"):
        want = list(hat[name.replace("_kd_", "_hat_")])
        want.insert(1, "pointer")
        at = max(i for i, k in enumerate(want) if k == "rnntOptions") + 2
        want[at:at] = ["int", "float"]
        assert sigs[name] == want, name


def test_code_objects_hold_exactly_the_table():
    I.assert_side_inventory(I.need_lib(LIB), F.expected_inventory())


def test_every_row_has_a_case():
    rows = F.predicted_rows()
    for obj, ks in F.expected_inventory().items():
        assert ks and all((obj, k) in rows for k in ks)
    ks = {k for _, k in rows}
    for tag in ("F32", "F64", "BF16", "F16"):
        for mode in (0, 1):
            for g in (4, 16, 64):
                assert "rnnt::kd_stats_kernel<rnnt::%s, %d, %d>" % (tag, g, mode) in ks
            for k in ("kd_grad_kernel", "kd_grad_elem_kernel"):
                assert "rnnt::%s<rnnt::%s, %d>" % (k, tag, mode) in ks
    # both sides of each threshold of the statistics rule, in bytes of a row
    sizes = {c["A"] * F.STORES[c["dtype"]][3] for c in F.CASES.values()}
    assert sizes >= {256, 260, 258, 2048, 2052, 2050}
    assert F.stats_group(256) == 4 and F.stats_group(258) == 16 and F.stats_group(2048) == 16 and F.stats_group(2050) == 64
    assert {c["A"] for c in F.CASES.values()} >= {2, 3, 5, 300, 1025, 5003}


def test_the_tables_rule_is_the_launchers():
    text = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_kd_impl.h")).read()
    assert "constexpr size_t kKdWideRowBytes = 2048;" in text and "kKdWideRowBytes)" in text
    side = open(os.path.join(ROOT, "warp-transducer_amd", "csrc", "rnnt_side_host.h")).read()
    assert "row_bytes <= 256 ? 4 : row_bytes <= wide_bytes ? 16 : 64" in side


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


def test_argument_checks_under_the_sanitizers():
    """make side-asan's program for this library: the host driver under ASan + UBSan, a stand-alone program, no GPU."""
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    pkg = os.path.join(ROOT, "warp-transducer_amd")
    built = subprocess.run(["make", "-C", pkg, "build/asan/test_kd_args"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([os.path.join(pkg, "build", "asan", "test_kd_args")], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "all refused" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "./build/asan/test_kd_args" in mk and "build/asan/test_kd_args" in mk.split("side-asan:")[1].split("\n")[0]


# ----------------------------------------------------------------------------- the Python module, without a device
def _cpu_args(A=5, U=3):
    z = torch.zeros(2, 4, U, A)
    return z, torch.zeros(2, 4, U, A), torch.ones(2, U - 1, dtype=torch.int32), torch.tensor([4, 3], dtype=torch.int32), \
        torch.tensor([U - 1, 1], dtype=torch.int32)


def test_python_argument_errors():
    from warprnnt_pytorch.kd import TransducerKDLoss, kd_loss_torch, rnnt_kd_loss
    z, w, lab, tl, ll = _cpu_args()
    with pytest.raises(ValueError, match="GPU"):
        rnnt_kd_loss(z, w, lab, tl, ll)
    with pytest.raises(ValueError, match="reduction"):
        rnnt_kd_loss(z, w, lab, tl, ll, reduction="max")
    for fn in (rnnt_kd_loss, kd_loss_torch):
        with pytest.raises(ValueError, match="mode"):
            fn(z, w, lab, tl, ll, mode="three")
        for tau in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature"):
                fn(z, w, lab, tl, ll, temperature=tau)
        with pytest.raises(ValueError, match="shape"):
            fn(z, w[:, :3], lab, tl, ll)
        with pytest.raises(TypeError, match="teacher"):
            fn(z, w.double(), lab, tl, ll)
        with pytest.raises(ValueError, match="contiguous"):
            fn(z, torch.zeros(2, 4, 5, 3).transpose(2, 3), lab, tl, ll)
        for blank in (-1, 5):
            with pytest.raises(ValueError, match="blank"):
                fn(z, w, lab, tl, ll, blank=blank)
        with pytest.raises(ValueError, match="column besides"):
            fn(z[..., :1].contiguous(), w[..., :1].contiguous(), lab, tl, ll)
    with pytest.raises(ValueError, match="device"):
        rnnt_kd_loss(z, w.to("meta"), lab, tl, ll)
    with pytest.raises(ValueError, match="mode"):
        TransducerKDLoss(mode="both")
    with pytest.raises(ValueError, match="reduction"):
        TransducerKDLoss(reduction="max")
    m = TransducerKDLoss(blank=3, mode="full", temperature=2, reduction="sum")
    assert (m.blank, m.mode, m.temperature, m.reduction) == (3, "full", 2.0, "sum")


def test_library_path_is_beside_the_main_library():
    from warprnnt_pytorch import _lib, kd
    assert kd.library_path() == os.path.join(os.path.dirname(_lib.library_path()), LIB)
    assert set(kd.__all__) == {"rnnt_kd_loss", "TransducerKDLoss", "kd_loss_torch", "library_path"}


def test_side_forward_default_is_unchanged():
    """_side.forward gained one keyword for the teacher; its six positional parameters and what it saves by default are what
    the seven other modules call it with."""
    from warprnnt_pytorch import _side
    params = list(inspect.signature(_side.forward).parameters.values())
    assert [p.name for p in params] == ["ctx", "logits", "labels", "workspace_size", "reduction", "call", "what", "also_save"]
    assert all(p.default is inspect.Parameter.empty for p in params[:7]) and params[7].default == ()
    from warprnnt_pytorch import hat
    src = inspect.getsource(hat._HAT.forward)
    assert "also_save" not in src and "_side.forward(ctx, logits, labels," in src
    assert "ctx.save_for_backward(logits, *also_save)" in inspect.getsource(_side.forward)
