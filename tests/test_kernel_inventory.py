"""No GPU: the kernels of the materialised path in the release build's code objects (warp-transducer_amd/lib/libwarprnnt.so)
against the committed table of tests/kernel_forms.py.  A kernel the build holds without a row -- a new form no case reaches --
fails, and so does a row naming a kernel the build no longer has.  Every row's case must reach its kernel under the release
rules (kernel_forms.predict); tests/test_gpu_kernel_forms.py runs the cases and checks on the GPU that they do."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import kernel_forms as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "warp-transducer_amd", "lib", "libwarprnnt.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def code_objects(path):
    """The gfx950 code objects (ELF images) of the offload bundles inside a shared library."""
    data = open(path, "rb").read()
    out, i = [], 0
    while True:
        i = data.find(MAGIC, i)
        if i < 0:
            return out
        count, = struct.unpack_from("<Q", data, i + len(MAGIC))
        p = i + len(MAGIC) + 8
        for _ in range(count):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "amdgcn" in triple and size and data[i + off:i + off + 4] == b"\x7fELF":
                out.append(data[i + off:i + off + size])
        i += len(MAGIC)


def kernel_names(elf, tmp_path, readelf, cxxfilt):
    """Demangled names (without the parameter list) of the kernel descriptors (*.kd) of one code object."""
    f = tmp_path / "co.elf"
    f.write_bytes(elf)
    syms = subprocess.run([readelf, "--symbols", "--wide", str(f)], capture_output=True, text=True, check=True).stdout
    mangled = sorted({ln.split()[-1][:-3] for ln in syms.splitlines() if ln.split() and ln.split()[-1].endswith(".kd")})
    dem = subprocess.run([cxxfilt], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.split("(")[0].replace("void ", "", 1).strip() for d in dem if d.strip()}


def classify(names):
    """Which object of the release build a code object is: f32 / f64 / h16 (materialised path), joint (out of scope)."""
    if any(n.split("<")[0].split("::")[-1].startswith("joint_") for n in names):
        return "joint"
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
        if obj != "joint":
            assert obj not in inv, "two code objects look like the %s translation unit" % obj
            inv[obj] = names
    return inv


def test_materialised_objects_present(build_inventory):
    assert set(build_inventory) == set(K.OBJECTS), sorted(build_inventory)


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
