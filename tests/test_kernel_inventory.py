"""No GPU: the kernels of the release build's code objects (warp-transducer_amd/lib/libwarprnnt.so) against the committed
tables of tests/kernel_forms.py (materialised path) and tests/joint_forms.py (additive joint and alignment).  A kernel the build holds without a row -- a new form no case reaches --
fails, and so does a row naming a kernel the build no longer has.  Every row's case must reach its kernel under the release
rules (kernel_forms.predict, joint_forms.predict_joint); tests/test_gpu_kernel_forms.py and tests/test_gpu_joint_forms.py run
the cases and check on the GPU that they do."""
import os
import shutil

import pytest

from tests import joint_forms as J
from tests import kernel_forms as K
from tests.inventory import LIBDIR, _tool, code_objects, kernel_names

LIB = os.path.join(LIBDIR, "libwarprnnt.so")


def classify(names):
    """Which object of the release build a code object is: f32 / f64 / h16 (materialised path), joint_f32 / joint_bf16 /
    joint_f16 (additive joint, by the store tag of its DF kernels)."""
    if any(n.split("<")[0].split("::")[-1].startswith("joint_") for n in names):
        objs = [obj for obj, tag, _ in J.JSTORES.values() if any(n.startswith("rnnt::joint_df_kernel<%s," % tag) for n in names)]
        return objs[0] if len(objs) == 1 else "unknown"
    for obj, tag in (("f32", "rnnt::F32"), ("f64", "rnnt::F64"), ("h16", "rnnt::BF16")):
        if any(n.startswith("rnnt::grad_flat_kernel<%s," % tag) for n in names):
            return obj
    return "unknown"


@pytest.fixture(scope="module")
def build_inventory(tmp_path_factory):
    readelf, cxxfilt = _tool("llvm-readelf"), _tool("llvm-cxxfilt") or shutil.which("c++filt")
    if readelf is None or cxxfilt is None:
        pytest.skip("needs llvm-readelf and a demangler (ROCm LLVM tools)")
    if not os.path.exists(LIB):
        pytest.skip("libwarprnnt.so is not built")
    tmp = tmp_path_factory.mktemp("co")
    inv = {}
    for elf in code_objects(LIB):
        names = kernel_names(elf, tmp, readelf, cxxfilt)
        obj = classify(names)
        assert obj != "unknown", sorted(names)[:10]
        assert obj not in inv, "two code objects look like the %s translation unit" % obj
        inv[obj] = names
    return inv


def test_materialised_objects_present(build_inventory):
    assert set(K.OBJECTS) <= set(build_inventory), sorted(build_inventory)


def test_joint_objects_present(build_inventory):
    """Exactly the three materialised and the three additive-joint objects, each recognised by its store tag."""
    assert set(build_inventory) == set(K.OBJECTS) | set(J.JOBJECTS), sorted(build_inventory)


@pytest.mark.parametrize("obj", sorted(K.OBJECTS))
def test_every_kernel_has_a_row_and_every_row_a_kernel(build_inventory, obj):
    built = build_inventory[obj]
    table = K.expected_inventory()[obj]
    missing_rows = sorted(built - set(table))
    stale_rows = sorted(set(table) - built)
    assert not missing_rows, "kernels of %s without a row in tests/kernel_forms.py: %s" % (K.OBJECTS[obj], missing_rows)
    assert not stale_rows, "rows naming kernels %s no longer holds: %s" % (K.OBJECTS[obj], stale_rows)


def test_every_row_is_reached_by_its_case():
    """kernel_forms.FORMS against the release rules (256 compute units: the MI355X); the GPU test repeats this with the
    device's own count and observes the launches."""
    reach = K.predicted_rows(256)
    for obj, kernel, case in K.FORMS:
        assert case in K.CASES, (kernel, case)
        assert case in reach.get((obj, kernel), []), "case %s does not reach %s under the release rules" % (case, kernel)
    # and every form a case reaches has a row (no case reaches an unlisted or an "unreachable" kernel)
    rows = {(o, k) for o, k, _ in K.FORMS}
    assert set(reach) <= rows, sorted(set(reach) - rows)
    forms = [(o, k) for o, k, _ in K.FORMS]
    assert len(forms) == len(set(forms))


def test_required_cases_are_present():
    """The cases the matrix must keep, whatever else changes."""
    rows = K.predicted_rows(256)
    for d, (obj, tag, lat, esz) in K.STORES.items():
        for sc, ps in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0)):
            assert (obj, "rnnt::grad_flat_kernel<%s, %d, 2, %d>" % (tag, sc, ps)) in rows
        for g in (1, 2, 4, 8, 16, 32):
            names = [c for c in rows.get((obj, "rnnt::row_stats_tile_kernel<%s, %d>" % (tag, g)), []) if K.CASES[c]["dtype"] == d]
            rbs = {K.CASES[c]["A"] * esz for c in names}
            lo = K.tile_limit(g // 2) + 1 if g > 1 else 1
            hi = K.tile_limit(g)
            assert hi // esz * esz in rbs and (g == 1 or -(-lo // esz) * esz in rbs), (d, g, sorted(rbs))   # both edges of G
        assert any(K.CASES[c]["A"] * esz == K.TILE_MAX_ROW_BYTES for c in rows[(obj, "rnnt::row_stats_tile_kernel<%s, 32>" % tag)])
    two = [c for c in K.CASES.values() if c.get("aux")]
    assert two and all(K.two_half_cut(c) == c["n0"] != c["N"] // 2 and c.get("scale") for c in two)
    assert all(K.CASES[c]["T"] + K.CASES[c]["U"] - 1 >= K.OVERLAP_MIN_DIAGONALS for c in (c["name"] for c in two))
    groups = [c for c in K.CASES.values() if K.coef_launches(c, 256) > 1]
    assert {K.STORES[c["dtype"]][0] for c in groups} == set(K.OBJECTS) and all(c["U"] <= 48 for c in groups)
    lin = {c["name"] for c in K.CASES.values() if c["N"] == "cus//2"}
    log = {c["name"] for c in K.CASES.values() if c["N"] == "cus//2+1"}
    assert len(lin) == len(log) == len(K.STORES)


# ----------------------------------------------------------------------------- the additive joint and the alignment kernels
@pytest.mark.parametrize("obj", sorted(J.JOBJECTS))
def test_joint_every_kernel_has_a_row_and_every_row_a_kernel(build_inventory, obj):
    built = build_inventory[obj]
    table = J.expected_inventory()[obj]
    missing_rows = sorted(built - set(table))
    stale_rows = sorted(set(table) - built)
    assert not missing_rows, "kernels of %s without a row in tests/joint_forms.py: %s" % (J.JOBJECTS[obj], missing_rows)
    assert not stale_rows, "rows naming kernels %s no longer holds: %s" % (J.JOBJECTS[obj], stale_rows)


def test_joint_every_row_is_reached_by_its_case():
    """joint_forms.FORMS against the release rules of run_gpu_joint (256 compute units); tests/test_gpu_joint_forms.py repeats
    this with the device's own count and observes the launches."""
    reach = J.predicted_rows(256)
    for obj, kernel, case in J.FORMS:
        assert case in J.JCASES, (kernel, case)
        assert case in reach.get((obj, kernel), []), "case %s does not reach %s under the release rules" % (case, kernel)
    rows = {(o, k) for o, k, _ in J.FORMS}
    assert set(reach) <= rows, sorted(set(reach) - rows)
    forms = [(o, k) for o, k, _ in J.FORMS]
    assert len(forms) == len(set(forms))
    # a form the table calls unreachable is reached by no case
    unreachable = {(obj, k) for obj, ks in J.expected_inventory().items() for k, why in ks.items() if why.startswith("unreachable")}
    assert not unreachable & set(reach), sorted(unreachable & set(reach))


def test_joint_rules_restate_the_source():
    """The constants predict_joint restates -- kJointZSmallA, the A >= 512 gates of the 16-bit matrix-core forms, the vocabulary
    split, the split DF / DG bounds, the release Tune defaults -- against the headers: a retune fails here before a GPU run."""
    assert J.source_constants() == J.restated_constants()


def test_joint_required_cases_are_present():
    """The boundaries the matrix must keep, whatever else changes: both sides of each threshold of run_gpu_joint."""
    sh = {n: K.case_shape(c, 256) for n, c in J.JCASES.items()}
    train = [n for n, c in J.JCASES.items() if c["entry"] not in ("align", "align_add")]
    for d in J.JSTORES:
        mine = [n for n in train if J.JCASES[n]["dtype"] == d]
        a = {sh[n][3] for n in mine}
        assert {J.JOINT_Z_SMALL_A, J.JOINT_Z_SMALL_A + 1, 63, 64} <= a, (d, sorted(a))
        assert {480, 488, 992, 1000} <= a                                    # ceil(A / 32) = 15 / 16, 31 / 32
        tiles = {sh[n][0] * ((sh[n][1] + 31) // 32) * ((sh[n][2] + 31) // 32) for n in mine}
        assert {1023, 1024, 4095, 4096} <= tiles
        assert {48, 49, 63, 64} <= {sh[n][2] for n in mine}
        assert {63, 64, 511, 512} <= {sh[n][1] for n in mine}
        if d != "f32":
            assert {504, 512} <= a
        for entry in ("guard", "masked32", "far"):
            assert any(J.JCASES[n].get("data") == entry for n in mine), (d, entry)
        assert any(J.JCASES[n]["N"] == "cus//2" for n in mine) and any(J.JCASES[n]["N"] == "cus//2+1" for n in mine)
    entries = {(c["entry"], c["dtype"]) for c in J.JCASES.values()}
    assert {("add", "f32"), ("twophase", "f32"), ("fastemit", "f32"), ("dt", "f32"), ("dt", "bf16"), ("dt", "f16")} <= entries
    assert {("align_add", d) for d in J.JSTORES} <= entries and {("align", d) for d in K.STORES} <= entries
    al = [n for n, c in J.JCASES.items() if c["entry"] in ("align", "align_add")]
    assert {64, 65, 1024} <= {sh[n][2] for n in al}
    assert any(sh[n][2] == 1024 and (sh[n][1] + 1024 - 1) > J.ALIGN_LDS_WORDS // J.ALIGN_MAX_WAVES for n in al)  # several chunks
    assert any(J.JCASES[n].get("data") == "planted" and sh[n][2] == 1024 for n in al)
