"""No GPU: the harness of the workspace contract (tests/ws_contract.py).  Its registry names exactly the sizing functions the
headers declare, so a new library cannot arrive without an adaptor; its judges refuse each planted fault -- one flipped bit in
one output, one changed guard byte -- and accept a run against itself; and the cases a library leaves out for size predict no
kernel that a kept case does not."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import inventory
from tests import ws_contract as W


def _outputs():
    rng = np.random.default_rng(0)
    return {"costs": rng.standard_normal(3).astype(np.float32), "grads": rng.standard_normal((3, 4, 2, 5)),
            "frames": torch.arange(6, dtype=torch.int32).view(3, 2),
            "half": torch.tensor(rng.standard_normal(7)).to(torch.bfloat16)}


def test_the_registry_names_the_declared_sizing_functions():
    headers = [os.path.basename(p) for p in glob.glob(os.path.join(inventory.ROOT, "include", "*.h"))]
    declared = {f for h in headers for f in inventory.declared(h) if re.match(r"get_workspace_size", f)}
    assert len(declared) >= 14
    assert set(W.REGISTRY) == declared, set(W.REGISTRY) ^ declared


def test_every_library_has_cases_and_every_case_a_dtype():
    for fn, lib in W.REGISTRY.items():
        cases = lib.cases()
        assert cases and all("dtype" in c for c in cases.values()), fn
        assert set(cases) | set(lib.left_out) == set(lib.all_cases()) and not set(cases) & set(lib.left_out), fn


def test_the_two_libraries_of_the_joint_table_share_it_out():
    """tests/joint_forms.py serves the additive joint and, with its `align` cases, the main library: each case once."""
    from tests import joint_forms as J
    main = {n[len("align/"):] for n in W.REGISTRY["get_workspace_size"].all_cases() if n.startswith("align/")}
    add = set(W.REGISTRY["get_workspace_size_add"].all_cases())
    assert main and not main & add and main | add == set(J.JCASES)


def test_a_run_agrees_with_itself():
    a, b = _outputs(), _outputs()
    assert W.differing(a, b) == []
    W.assert_same(a, b, "itself")
    nan = {"g": np.array([np.nan, 1.0])}
    assert W.differing(nan, {"g": np.array([np.nan, 1.0])}) == []            # NaN against the same NaN: the same bits


@pytest.mark.parametrize("name", sorted(_outputs()))
def test_one_flipped_bit_is_refused(name):
    want, got = _outputs(), _outputs()
    v = got[name]
    raw = v.view(np.uint8) if isinstance(v, np.ndarray) else v.view(torch.uint8)
    raw.reshape(-1)[raw.reshape(-1).shape[0] // 2] ^= 1                       # the lowest bit of one byte in the middle
    assert W.differing(got, want) == [name]
    with pytest.raises(AssertionError, match=name):
        W.assert_same(got, want, "planted")


def test_other_departures_are_refused():
    want = _outputs()
    assert W.differing({k: v for k, v in want.items() if k != "grads"}, want) == ["grads"]                # an output missing
    assert W.differing(dict(want, costs=want["costs"].astype(np.float64)), want) == ["costs"]               # another type
    assert W.differing(dict(want, frames=want["frames"].view(2, 3)), want) == ["frames"]                    # another shape
    assert W.differing(dict(want, costs=-want["costs"] * 0.0), dict(want, costs=want["costs"] * 0.0)) == ["costs"]    # -0.0


@pytest.mark.parametrize("shift", [0, W.SHIFT])
@pytest.mark.parametrize("at", ["first", "before", "behind", "last"])
def test_one_changed_guard_byte_is_refused(shift, at):
    w = W.Workspace(1000, shift, fill=0xFF, device="cpu")
    assert w.ws.numel() == 1000 and w.guards_intact() and bool((w.ws == 0xFF).all())
    w.assert_guards("untouched")
    w.ws.fill_(7)                                                              # the workspace itself is the call's to write
    assert w.guards_intact()
    i = {"first": 0, "before": w.lo - 1, "behind": w.hi, "last": w.buf.numel() - 1}[at]
    w.buf[i] ^= 1
    assert not w.guards_intact()
    with pytest.raises(AssertionError, match="in front of" if at in ("first", "before") else "behind"):
        w.assert_guards("planted")


@pytest.mark.parametrize("size_fn", sorted(W.REGISTRY))
def test_left_out_cases_stay_covered(size_fn):
    """A case may be left out for size only: at W.LIMIT elements or more, and every kernel it predicts predicted by a kept one."""
    lib = W.REGISTRY[size_fn]
    missing, small = W.uncovered(lib)
    assert set(missing) == set(lib.left_out)
    assert not any(missing.values()), missing
    assert not small, small


def test_the_rule_refuses_a_case_that_nothing_else_covers():
    lib = W.REGISTRY["get_workspace_size_mono"]
    planted = W.Library(lib.size_fn, lib.tables, None, left_out=lib.left_out + ("f64_u65", "f64_u130"))
    missing, small = W.uncovered(planted)
    assert missing["f64_u130"] and small == ["f64_u65", "f64_u130"]          # (the fp64 block lattice: only u65, u130, u1100)


def test_scales_are_per_sample_and_not_one():
    for which in (1, 2):
        s = W.scales(5, which)
        assert s.shape == (5,) and (s != 1).all() and len(set(s)) > 1
    assert not np.array_equal(W.scales(5, 1), W.scales(5, 2))
