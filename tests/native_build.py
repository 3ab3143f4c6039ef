"""Build and run the stand-alone host programs of tests/native/ (the headers' emulators), once.

Every caller keeps the command line it always had; what differs between them is an argument here:

    [compiler, opt, -std=c++17, (-ffp-contract=off), (-Wall), (-Werror), (-x c++), *extra, -o, exe, source]

-ffp-contract=off is how the library itself is built (lagomorph_amd/build.py): the double expressions keep their order."""
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
CXX_OR_HIPCC = CXX or ("hipcc" if shutil.which("hipcc") else None)   # for programs of host code only, which hipcc compiles as C++ (-x c++)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no C++ compiler available")
needs_cxx_or_hipcc = pytest.mark.skipif(CXX_OR_HIPCC is None, reason="no C++ compiler available")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
GFX950 = ("--offload-arch=gfx950",)


def build(tmp_path, source, opt="-O2", fp_contract_off=True, werror=True, extra=(), compiler=None, name=None, wall=True):
    """Compile tests/native/<source> into tmp_path/<name> (the source's stem unless given); returns the program's path."""
    compiler = compiler or CXX
    exe = str(tmp_path / (name or os.path.splitext(source)[0]))
    cmd = [compiler, opt, "-std=c++17"]
    cmd += ["-ffp-contract=off"] if fp_contract_off else []
    cmd += ["-Wall"] if wall else []
    cmd += ["-Werror"] if werror else []
    cmd += ["-x", "c++"] if compiler == "hipcc" and source.endswith(".cpp") else []
    subprocess.run([*cmd, *extra, "-o", exe, os.path.join(NATIVE, source)], check=True, timeout=600)
    return exe


def run(exe, *args, stdin=None, timeout=600, quiet=False):
    """Run the program; exit status 0 is asserted, and with quiet=True an empty stderr (what a sanitizer writes to)."""
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and not (quiet and r.stderr.strip()), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r
