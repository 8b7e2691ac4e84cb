"""No GPU: the Python layer of the four side libraries (warprnnt_pytorch.pruned / .tdt / .hat / .mblank over _side.py).  Their
ctypes tables against the headers' declarations -- names, restype, the number of arguments and the kind of each -- with planted
faults to show that the comparison refuses them; the per-library workspace-size cache against the entries themselves; the
ImportError of a missing library; and the texts of the refusals a CPU tensor can reach."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import pytest
import torch

from tests import inventory as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = {   # module: (library, header, the loss in its messages, its workspace entry, that entry's integer after N)
    "pruned": ("libwarprnnt_pruned.so", "rnnt_pruned.h", "the pruned loss", "get_workspace_size_pruned", ()),
    "tdt": ("libwarprnnt_tdt.so", "rnnt_tdt.h", "the TDT loss", "get_workspace_size_tdt", (3,)),
    "hat": ("libwarprnnt_hat.so", "rnnt_hat.h", "the HAT loss", "get_workspace_size_hat", ()),
    "mblank": ("libwarprnnt_mblank.so", "rnnt_mblank.h", "the multi-blank loss", "get_workspace_size_mblank", (2,)),
}


def _module(name):
    return importlib.import_module("warprnnt_pytorch." + name)


# ----------------------------------------------------------------------------- the ctypes tables against the headers
@pytest.mark.parametrize("name", sorted(SIDE))
def test_python_bindings_match_the_header(name):
    header = SIDE[name][1]
    sigs = I.declared_signatures(header)
    assert set(sigs) == I.declared(header) and all(sigs.values())          # (the parser saw every declaration whole)
    assert I.binding_faults(_module(name).EXPORTS, header) == []


def _swap_int_and_float(args):
    i = args.index(C.c_float)
    assert args[i - 1] is C.c_int
    args[i - 1], args[i] = args[i], args[i - 1]


def _drop_the_argument_before_the_options(args):
    from warprnnt_pytorch import _lib
    del args[args.index(_lib.rnntOptions) - 1]


def _pointer_for_the_options(args):
    from warprnnt_pytorch import _lib
    args[args.index(_lib.rnntOptions)] = C.c_void_p


@pytest.mark.parametrize("plant", [_swap_int_and_float, _drop_the_argument_before_the_options, _pointer_for_the_options])
def test_a_planted_fault_in_a_table_is_refused(plant):
    from warprnnt_pytorch import tdt
    table = {name: (res, list(args)) for name, (res, args) in tdt.EXPORTS.items()}
    assert I.binding_faults(table, "rnnt_tdt.h") == []
    plant(table["compute_tdt_loss_fwd"][1])
    faults = I.binding_faults(table, "rnnt_tdt.h")
    assert faults and all(f.startswith("compute_tdt_loss_fwd:") for f in faults), faults


def test_a_wrong_restype_or_name_is_refused():
    from warprnnt_pytorch import hat
    table = dict(hat.EXPORTS)
    table["compute_hat_loss_bwd"] = (None, hat.EXPORTS["compute_hat_loss_bwd"][1])
    assert I.binding_faults(table, "rnnt_hat.h") == ["compute_hat_loss_bwd: restype None"]
    table = dict(hat.EXPORTS)
    table["compute_hat_loss_bwd2"] = table.pop("compute_hat_loss_bwd")
    assert len(I.binding_faults(table, "rnnt_hat.h")) == 2


# ----------------------------------------------------------------------------- one workspace-size cache per library
def test_workspace_sizes_are_cached_per_library():
    """The four lookups interleaved at one common (maxT, maxU, N, dtype): a cache shared across the libraries would hand one loss
    another's size -- an out-of-bounds write on the device.  The entries are host arithmetic, so no GPU is needed."""
    from warprnnt_pytorch import _lib
    for lib, *_ in SIDE.values():
        I.need_lib(lib)
    T, U, N, code = 8, 4, 2, _lib.DT_F32

    def direct(name):
        n = C.c_size_t(0)
        entry, extra = SIDE[name][3], SIDE[name][4]
        assert getattr(_module(name).lib(), entry)(T, U, N, *extra, code, C.byref(n)) == 0
        return n.value
    want = {name: direct(name) for name in SIDE}
    assert all(v > 0 for v in want.values()), want
    for _ in range(2):
        got = {name: _module(name).workspace_bytes(T, U, N, *SIDE[name][4], code) for name in sorted(SIDE)}
        assert got == want


# ----------------------------------------------------------------------------- a missing library
def test_a_missing_library_is_an_import_error(tmp_path):
    """WARP_RNNT_PATH names a directory without libraries: `import warprnnt_pytorch` works, every side module's lib() raises."""
    code = ("import sys\n"
            "sys.path.insert(0, %r)\n"
            "import warprnnt_pytorch\n"
            "for name in %r:\n"
            "    module = __import__('warprnnt_pytorch.' + name, fromlist=['lib'])\n"
            "    try:\n"
            "        module.lib()\n"
            "    except ImportError as e:\n"
            "        print(e)\n"
            "    else:\n"
            "        sys.exit('%%s.lib() loaded something' %% name)\n" % (os.path.join(ROOT, "warp-transducer_amd"), sorted(SIDE)))
    env = dict(os.environ, WARP_RNNT_PATH=str(tmp_path))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    want = ["%s not found at %s -- build it with `make -C warp-transducer_amd`. There is no fallback for %s."
            % (SIDE[name][0], tmp_path / SIDE[name][0], SIDE[name][2]) for name in sorted(SIDE)]
    assert out.stdout.splitlines() == want


# ----------------------------------------------------------------------------- refusals a CPU tensor reaches
def _loss(name, logits, labels, act_lens, label_lens):
    """The functional form of a side loss on (N, T, U, A) = (2, 3, 2, 5) inputs (pruned: S = 2 and ranges (N, T))."""
    module = _module(name)
    if name == "pruned":
        return module.rnnt_loss_pruned(logits, labels, act_lens, label_lens, torch.zeros((2, 3), dtype=torch.int32))
    if name == "tdt":
        return module.rnnt_loss_tdt(logits, labels, act_lens, label_lens, (0, 1))
    if name == "hat":
        return module.rnnt_loss_hat(logits, labels, act_lens, label_lens)
    return module.rnnt_loss_mblank(logits, labels, act_lens, label_lens, (2,), blank=4)


def _inputs():
    return [torch.zeros(2, 3, 2, 5), torch.ones((2, 1), dtype=torch.int32), torch.full((2,), 3, dtype=torch.int32),
            torch.ones(2, dtype=torch.int32)]


REFUSALS = [   # (which input, what becomes of it, the exception, its text)
    (1, lambda t: t.long(), TypeError, "labels must be torch.int32"),
    (2, lambda t: t.long(), TypeError, "lengths must be torch.int32"),
    (3, lambda t: t.long(), TypeError, "label_lengths must be torch.int32"),
    (0, lambda t: t.transpose(1, 2), ValueError, "logits must be contiguous"),
    (1, lambda t: t.expand(2, 3)[:, ::2], ValueError, "labels must be contiguous"),
    (0, lambda t: t[0], ValueError, "logits must be 4D"),
    (1, lambda t: t[:, 0], ValueError, "labels must be 2D"),
    (2, lambda t: t[:, None].contiguous(), ValueError, "lengths must be 1D"),
    (3, lambda t: t[:, None].contiguous(), ValueError, "label_lengths must be 1D"),
]


@pytest.mark.parametrize("name", sorted(SIDE))
def test_the_common_refusals_and_their_texts(name):
    for which, change, exc, text in REFUSALS:
        args = _inputs()
        args[which] = change(args[which])
        with pytest.raises(exc) as e:
            _loss(name, *args)
        assert str(e.value) == text, (which, text)


def test_cpu_tensors_are_refused_in_each_modules_words():
    want = {"pruned": "the pruned loss runs on the GPU only",
            "tdt": "the TDT loss runs on the GPU only: logits are on cpu",
            "hat": "the HAT loss runs on the GPU only: logits are on cpu",
            "mblank": "the multi-blank loss runs on the GPU only: logits are on cpu"}
    for name in sorted(SIDE):
        with pytest.raises(ValueError) as e:
            _loss(name, *_inputs())
        assert str(e.value) == want[name]
