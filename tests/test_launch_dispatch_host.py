"""Host check of the launch dispatch helpers (no GPU needed).

Every kernel family of the library is a template over a few flags and small integers known only at run time;
lagomorph_amd/csrc/launch.hpp (with_flags, with_dim, with_int) turns them into the template arguments.  A mix-up there
selects a wrong instantiation silently.  tests/native/launch_dispatch_emul.cpp includes the header with a plain C++17
compiler and checks, for 1 to 4 flags over every runtime combination, alone and nested inside with_dim and
with_int<256, 512, 1024>: the compile-time values received equal the runtime values passed, position by position; f is
called exactly once per dispatch; with_int returns false without calling f for a value outside its list."""
import re

import native_build

pytestmark = native_build.needs_cxx_or_hipcc


def test_dispatch_values_positions_and_single_call(tmp_path):
    # (as host code only: the dispatch part needs no HIP)
    r = native_build.run(native_build.build(tmp_path, "launch_dispatch_emul.cpp", "-O1", fp_contract_off=False, compiler=native_build.CXX_OR_HIPCC))
    m = re.search(r"(\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 500, r.stdout
