"""Host check of the launch dispatch helpers (no GPU needed).

Every kernel family of the library is a template over a few flags and small integers known only at run time;
lagomorph_amd/csrc/launch.hpp (with_flags, with_dim, with_int) turns them into the template arguments.  A mix-up there
selects a wrong instantiation silently.  tests/native/launch_dispatch_emul.cpp includes the header with a plain C++17
compiler and checks, for 1 to 4 flags over every runtime combination, alone and nested inside with_dim and
with_int<256, 512, 1024>: the compile-time values received equal the runtime values passed, position by position; f is
called exactly once per dispatch; with_int returns false without calling f for a value outside its list."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason="no C++ compiler available")


def test_dispatch_values_positions_and_single_call(tmp_path):
    exe = str(tmp_path / "launch_dispatch_emul")
    src = os.path.join(HERE, "native", "launch_dispatch_emul.cpp")
    lang = ["-x", "c++"] if CXX == "hipcc" else []   # (as host code only: the dispatch part needs no HIP)
    subprocess.run([CXX, "-O1", "-std=c++17", "-Wall", "-Werror", *lang, "-o", exe, src], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 500, r.stdout
