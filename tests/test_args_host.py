"""Host check of the entry points' argument frame (no GPU needed).

lagomorph_amd/csrc/args.hpp holds, once, what every newer entry point checks before its first device call: the checked
volume (dim, the 2D remap, negative extents and counts, extents of 2^31 or more, the plane limit), the extent rules of
make_geom, and the rule that no output overlaps an input or another output.  tests/native/args_emul.cpp includes the
header with a plain C++17 compiler, stubs fail_invalid so that the message is recorded, and compares

  * check_volume for dim in {-3, 0, 1, 2, 3, 4}, every triple of 20 extents from -1 to INT64_MAX and each plane limit in
    use (2^29 elements, 2^32 bytes of 4- and 8-byte elements, 2^30 voxels) with a verdict computed in unsigned __int128:
    accepted or rejected, the remapped extents and nvox, and which condition fired (by its message);
  * geom_volume -- what make_geom(g, dim, nn, nx, ny, nz) accepts -- over the same triples, among them those whose
    int64_t product wraps to a small value ((2^32 + 1, 2^32 - 1, 1) and the like: accepted before this header, rejected
    now), and the shapes at the 2^29 limit: (1, 2^14, 2^14) is 2^28 voxels and passes, (1, 2^15, 2^14) and
    (2^9, 2^10, 2^10) are 2^29 and do not, (2^9, 2^10, 2^10 - 1) passes;
  * any_overlap for two outputs and two inputs, pointers 0..12 (0: null) and sizes 0..4 bytes, every combination against
    the sets of byte addresses; a null or empty span never causes a rejection;
  * check_gather's byte counts, null and overlap rules on a few hand-made layouts."""
import re

import native_build

pytestmark = native_build.needs_cxx_or_hipcc


def test_volume_geom_and_overlap_rules_against_wide_references(tmp_path):
    # (as host code only: this part of the header needs no HIP)
    r = native_build.run(native_build.build(tmp_path, "args_emul.cpp", "-O1", fp_contract_off=False, compiler=native_build.CXX_OR_HIPCC))
    m = re.search(r"(\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 17_000_000, r.stdout
