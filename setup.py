"""pip-installable `warprnnt_pytorch` for the MI355X library (the role of the reference's pytorch_binding/setup.py:1-60).

    pip install . --no-build-isolation          # builds libwarprnnt.so with hipcc (gfx950) and the extension module with g++
    WARP_RNNT_PATH=/dir/with/libwarprnnt.so pip install . --no-build-isolation      # a prebuilt library, as the reference asks for

The installed package is self-contained: warprnnt_pytorch/{*.py, _warp_rnnt_ext*.so, lib/libwarprnnt.so, include/rnnt.h}, and
lib/libwarprnnt_pruned.so + include/rnnt_pruned.h for warprnnt_pytorch.pruned, lib/libwarprnnt_tdt.so + include/rnnt_tdt.h
for warprnnt_pytorch.tdt, lib/libwarprnnt_hat.so + include/rnnt_hat.h for warprnnt_pytorch.hat, lib/libwarprnnt_mblank.so +
include/rnnt_mblank.h for warprnnt_pytorch.mblank, lib/libwarprnnt_tdt_align.so + include/rnnt_tdt_align.h for
warprnnt_pytorch.tdt_align, lib/libwarprnnt_mono.so + include/rnnt_mono.h for warprnnt_pytorch.mono, lib/libwarprnnt_ar.so +
include/rnnt_ar.h for warprnnt_pytorch.ar, lib/libwarprnnt_kd.so + include/rnnt_kd.h for warprnnt_pytorch.kd,
lib/libwarprnnt_delay.so + include/rnnt_delay.h for warprnnt_pytorch.delay, lib/libwarprnnt_mi.so + include/rnnt_mi.h for
warprnnt_pytorch.mi, lib/libwarprnnt_pstream.so + include/rnnt_pstream.h for warprnnt_pytorch.pstream and
lib/libwarprnnt_joiner.so + include/rnnt_joiner.h for warprnnt_pytorch.joiner, lib/libwarprnnt_logprobs.so +
include/rnnt_logprobs.h for warprnnt_pytorch.logprobs, lib/libwarprnnt_bestpath.so + include/rnnt_bestpath.h for
warprnnt_pytorch.bestpath when those libraries
were built (or lie beside a WARP_RNNT_PATH library);
no sys.path edits, no environment variables at run time (a WARP_RNNT_PATH naming ANOTHER library at run time is honoured by switching to
the ctypes loader: the compiled module is linked to the library it was built with).
torch must be importable at build time (--no-build-isolation), exactly as for the reference's setup.py, which imports it.
"""
import importlib.util
import os
import shutil
import subprocess
import sys

from setuptools import setup
from setuptools.command.build_py import build_py
from setuptools.command.develop import develop
from setuptools.dist import Distribution

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG_SRC = os.path.join(ROOT, "warp-transducer_amd", "warprnnt_pytorch")
SIDE = ("pruned", "tdt", "hat", "mblank", "tdt_align", "mono", "ar", "kd", "delay") + ("mi",) + ("pstream",) + ("joiner",) + ("logprobs",) + ("bestpath",) + ("expect",) + ("sample",) + ("ranges",)      # warprnnt_pytorch.NAME loads lib/libwarprnnt_NAME.so (include/rnnt_NAME.h)
SIDE_LIBS = ["libwarprnnt_%s.so" % name for name in SIDE]
MAKE_LIBS = (["make", "-j3", "-C", os.path.join(ROOT, "warp-transducer_amd"), "lib/libwarprnnt.so"]
             + ["lib/" + so for so in SIDE_LIBS])


class BinaryDistribution(Distribution):
    def has_ext_modules(self):          # platform wheel: the package carries two shared objects
        return True


class build_native(build_py):
    """Python sources, then the native pair into the package directory of the build tree."""

    def run(self):
        super().run()
        if getattr(self, "editable_mode", False):
            # PEP 660 (`pip install -e .` with setuptools >= 64, editable_wheel): the package is imported from the SOURCE tree, so
            # the native pair must be built there -- build_lib is a temporary directory nothing will ever import from
            _build_in_tree()
            return
        pkg_out = os.path.join(self.build_lib, "warprnnt_pytorch")
        lib_out = os.path.join(pkg_out, "lib")
        os.makedirs(lib_out, exist_ok=True)
        prebuilt = os.environ.get("WARP_RNNT_PATH")
        if prebuilt:
            src = os.path.join(prebuilt, "libwarprnnt.so") if os.path.isdir(prebuilt) else prebuilt
            if not os.path.exists(src):
                raise SystemExit("Could not find libwarprnnt.so in %s (WARP_RNNT_PATH)" % prebuilt)
        else:
            subprocess.run(MAKE_LIBS, check=True)
            src = os.path.join(ROOT, "warp-transducer_amd", "lib", "libwarprnnt.so")
        shutil.copy2(src, os.path.join(lib_out, "libwarprnnt.so"))
        # the side losses' libraries (their modules load them on first use): beside libwarprnnt.so when built or handed over;
        # without one the package installs and everything else works
        for extra in SIDE_LIBS:
            path = os.path.join(os.path.dirname(src), extra)
            if os.path.exists(path):
                shutil.copy2(path, os.path.join(lib_out, extra))
        inc_out = os.path.join(pkg_out, "include")
        os.makedirs(inc_out, exist_ok=True)
        for header in ["rnnt.h"] + ["rnnt_%s.h" % name for name in SIDE]:
            shutil.copy2(os.path.join(ROOT, "include", header), os.path.join(inc_out, header))
        spec = importlib.util.spec_from_file_location("_warprnnt_build_ext", os.path.join(PKG_SRC, "build_ext.py"))
        be = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(be)
        be.build(force=True, lib_dir=lib_out, out_dir=pkg_out)


def _build_in_tree():
    if not os.environ.get("WARP_RNNT_PATH"):
        subprocess.run(MAKE_LIBS, check=True)
    subprocess.run([sys.executable, os.path.join(PKG_SRC, "build_ext.py")], check=True)


class develop_native(develop):
    """`pip install -e .` / `setup.py develop`: the package runs from the source tree, so the native pair is built IN the
    tree (what __graft_entry__.build() does) -- an editable install without it would silently fall back to the ctypes
    loader, or find no library at all."""

    def run(self):
        _build_in_tree()
        super().run()


setup(
    name="warprnnt_pytorch",
    version="0.4.0",
    description="RNN-Transducer loss for AMD MI355X (gfx950): drop-in for HawkAaron/warp-transducer's PyTorch binding",
    packages=["warprnnt_pytorch"],
    package_dir={"warprnnt_pytorch": os.path.relpath(PKG_SRC, ROOT)},
    python_requires=">=3.8",
    cmdclass={"build_py": build_native, "develop": develop_native},
    distclass=BinaryDistribution,
    zip_safe=False,
)
