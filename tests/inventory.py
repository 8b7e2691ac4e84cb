"""No GPU: what the built shared libraries hold -- the kernels of their gfx950 code objects, their exported symbols -- and
what the headers declare, for the tests that compare them with the committed tables."""
import os
import pathlib
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "warp-transducer_amd", "lib")
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


def need_lib(name):
    """The path of a built library of warp-transducer_amd/lib; skips the test when it is not built."""
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        pytest.skip("%s is not built" % name)
    return path


def exports(path):
    """The symbols a shared library defines and exports."""
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-2] in ("T", "W")}


def declared(header):
    """The functions a header of include/ declares."""
    return set(re.findall(r"^rnntStatus_t\s+(\w+)\(", open(os.path.join(ROOT, "include", header)).read(), re.M))


def declared_signatures(header):
    """{function: [kind of each parameter]} of the functions a header of include/ declares, in the kinds a ctypes table has to
    tell apart: 'pointer', 'size_t*', 'int', 'float', 'rnntOptions'.  A parameter of any other type is an error."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"^rnntStatus_t\s+(\w+)\(([^()]*)\)\s*;", text, re.M):
        kinds = []
        for p in params.split(","):
            ctype = re.sub(r"\bconst\b|\w+\s*$|\s", "", p)                              # the type without the parameter's name
            if ctype.endswith("*"):
                kinds.append("size_t*" if ctype == "size_t*" else "pointer")
            elif ctype in ("int", "float", "rnntOptions"):
                kinds.append(ctype)
            else:
                raise ValueError("%s: %s(... %s ...): a parameter type this parser does not know" % (header, name, p.strip()))
        out[name] = kinds
    return out


def binding_faults(exports, header):
    """Where a ctypes table {name: (restype, argtypes)} departs from the header's declarations: names, restype c_int, the
    number of arguments and the kind of each, position by position.  [] when it matches."""
    import ctypes as C
    from warprnnt_pytorch import _lib
    ctype = {"pointer": C.c_void_p, "size_t*": C.POINTER(C.c_size_t), "int": C.c_int, "float": C.c_float,
             "rnntOptions": _lib.rnntOptions}
    want = declared_signatures(header)
    faults = ["%s: only in %s" % (n, "the table" if n in exports else header) for n in sorted(set(exports) ^ set(want))]
    for name in sorted(set(exports) & set(want)):
        res, args = exports[name]
        if res is not C.c_int:
            faults.append("%s: restype %r" % (name, res))
        if len(args) != len(want[name]):
            faults.append("%s: %d arguments, %s declares %d" % (name, len(args), header, len(want[name])))
        faults += ["%s: argument %d is %r, %s declares %s" % (name, i, a, header, k)
                   for i, (a, k) in enumerate(zip(args, want[name])) if a is not ctype[k]]
    return faults


def side_inventory(lib):
    """{f32 | f64 | h16: kernel names} of a side library's three code objects, each recognised by its store tag."""
    readelf, cxxfilt = _tool("llvm-readelf"), _tool("llvm-cxxfilt") or shutil.which("c++filt")
    if readelf is None or cxxfilt is None:
        pytest.skip("needs llvm-readelf and a demangler")
    tmp = pathlib.Path(tempfile.mkdtemp())
    got = {}
    for elf in code_objects(lib):
        names = kernel_names(elf, tmp, readelf, cxxfilt)
        obj = "f64" if any("F64" in n for n in names) else "h16" if any("BF16" in n for n in names) else "f32"
        assert obj not in got
        got[obj] = names
    return got


def assert_side_inventory(lib, want):
    """The code objects of `lib` hold exactly the kernels of `want` (a form table's expected_inventory())."""
    got = side_inventory(lib)
    assert set(got) == set(want)
    for obj in want:
        assert got[obj] == want[obj], (obj, sorted(got[obj] - want[obj]), sorted(want[obj] - got[obj]))
