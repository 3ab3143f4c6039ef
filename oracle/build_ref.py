"""TEST INFRASTRUCTURE ONLY -- build oracle/_ref from the reference's own sources.

The only part of the reference that is plain C++ (everything else is CUDA,
which this image cannot compile: no nvcc, no cuda headers) is
``lagomorph/extension/cpu/affine.cpp``.  It is compiled here from where it lies
under /root/reference into ``oracle/_ref/lagomorph_ref_cpu.so`` (git-ignored,
travels to the GPU box with the snapshot).  No reference source is copied.

Usage: python oracle/build_ref.py        (no-op with a message when the
reference tree is absent, e.g. on the GPU box)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LAGOMORPH_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "lagomorph", "extension", "cpu", "affine.cpp")
INC = os.path.join(REF, "lagomorph", "extension", "include")
OUT = os.path.join(HERE, "_ref")
NAME = "lagomorph_ref_cpu"


def built_path():
    return os.path.join(OUT, NAME + ".so")


def build(verbose=False):
    if not os.path.exists(SRC):
        print(f"[oracle/_ref] reference tree not present ({SRC}); keeping prebuilt files if any")
        return os.path.exists(built_path())
    if os.path.exists(built_path()) and os.path.getmtime(built_path()) >= max(
        os.path.getmtime(SRC), os.path.getmtime(os.path.join(HERE, "ref_cpu_binding.cpp")), os.path.getmtime(os.path.join(INC, "interp.h"))
    ):
        return True
    os.makedirs(OUT, exist_ok=True)
    from torch.utils.cpp_extension import load

    load(
        name=NAME,
        sources=[os.path.join(HERE, "ref_cpu_binding.cpp")],
        extra_include_paths=[INC],
        extra_cflags=["-O2", "-w", "-ffp-contract=off", f'-DLAGOMORPH_REF_CPU_AFFINE=\\"{SRC}\\"'],
        build_directory=OUT,
        with_cuda=False,
        verbose=verbose,
    )
    return os.path.exists(built_path())


EXT_SRC = os.path.join(REF, "lagomorph", "extension", "extension.cpp")
FWD_SRC = os.path.join(HERE, "..", "tests", "native", "lagomorph_ext_forwarders.cpp")
NAME_B = "lagomorph_ext_optionb"


# How the option-B module is linked.  It names no path to liblagomorph_hip.so: its lago_* symbols are resolved when it is
# loaded, from the library load_option_b() has loaded RTLD_GLOBAL first, so a prebuilt module works wherever the tree
# lies.  The recipe is stamped beside the module; a module without the same stamp (an older recipe linked the library
# by absolute path) is rebuilt, whatever its age.
LDFLAGS_B = ["-L/opt/rocm/lib", "-lamdhip64", "-lc10_hip", "-ltorch_hip"]
LIB_B = os.path.abspath(os.path.join(HERE, "..", "lagomorph_amd", "_lib", "liblagomorph_hip.so"))


def built_path_b():
    return os.path.join(OUT, NAME_B + ".so")


def _stamp_path_b():
    return os.path.join(OUT, NAME_B + ".ldflags")


def _stamp_matches_b():
    try:
        with open(_stamp_path_b()) as f:
            return f.read() == " ".join(LDFLAGS_B)
    except OSError:
        return False


def _preload_lib_b():
    """Load liblagomorph_hip.so RTLD_GLOBAL: the option-B module's lago_* symbols are resolved from it."""
    import ctypes

    ctypes.CDLL(LIB_B, mode=ctypes.RTLD_GLOBAL)


def build_option_b(verbose=False):
    """INTEGRATION.md option B as a real build: the reference's OWN extension.cpp (argument checks +
    PYBIND11_MODULE, compiled from where it lies) + its cpu/affine.cpp + tests/native/
    lagomorph_ext_forwarders.cpp in place of the four cuda/*.cu files, calling into liblagomorph_hip.so
    (LDFLAGS_B).  The result is the reference's `lagomorph_ext` pybind module running on the HIP
    kernels; tests/test_option_b.py imports it on the GPU box.  Test infrastructure (it contains compiled
    reference code), hence under oracle/_ref."""
    if not os.path.exists(EXT_SRC):
        print(f"[oracle/_ref] reference tree not present ({EXT_SRC}); keeping prebuilt files if any")
        return os.path.exists(built_path_b())
    deps = [EXT_SRC, SRC, FWD_SRC, os.path.join(HERE, "ref_cpu_binding.cpp"),
            os.path.join(HERE, "..", "include", "lagomorph_hip.h")]
    if os.path.exists(built_path_b()) and _stamp_matches_b() and \
            os.path.getmtime(built_path_b()) >= max(os.path.getmtime(d) for d in deps):
        return True
    os.makedirs(OUT, exist_ok=True)
    for stale in (built_path_b(), _stamp_path_b()):
        if os.path.exists(stale):
            os.remove(stale)
    from torch.utils.cpp_extension import load

    if not os.path.exists(LIB_B):  # (this recipe may run before anything has built the library)
        _load_by_path("lagomorph_amd_build", os.path.join(HERE, "..", "lagomorph_amd", "build.py")).build()
    _preload_lib_b()  # load() imports the module it has built
    load(
        name=NAME_B,
        sources=[EXT_SRC, FWD_SRC, os.path.join(HERE, "ref_cpu_binding.cpp")],
        extra_include_paths=[INC, os.path.join(HERE, "..", "include"), "/opt/rocm/include"],
        extra_cflags=["-O2", "-w", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DLAGOMORPH_REF_NO_MODULE",
                      f'-DLAGOMORPH_REF_CPU_AFFINE=\\"{SRC}\\"'],
        extra_ldflags=list(LDFLAGS_B),  # (load() appends to the list it is given)
        build_directory=OUT,
        with_cuda=False,
        verbose=verbose,
    )
    if os.path.exists(built_path_b()):
        with open(_stamp_path_b(), "w") as f:
            f.write(" ".join(LDFLAGS_B))
    return os.path.exists(built_path_b())


def load_option_b():
    import torch  # noqa: F401

    p = built_path_b()
    if not os.path.exists(p):
        return None
    _preload_lib_b()
    tmp = None
    if any(os.path.basename(n) == os.path.basename(LIB_B) for n in _needed(p)):
        # a module prebuilt by an earlier recipe names the library as a dependency (by absolute path, or by name with
        # an rpath), which the loader cannot follow once the tree lies elsewhere: load a copy without that entry --
        # its symbols then come from the preload, as for a module built by LDFLAGS_B
        import tempfile

        tmp = tempfile.mkdtemp(prefix="optionb_")
        p = os.path.join(tmp, os.path.basename(p))
        with open(p, "wb") as f:
            f.write(_drop_needed(built_path_b(), os.path.basename(LIB_B)))
    try:
        mod = _load_by_path(NAME_B, p)
    finally:
        if tmp is not None:
            import shutil

            shutil.rmtree(tmp, ignore_errors=True)
    return mod


def _load_by_path(name, path):
    import importlib.util

    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dynamic(data):
    """(file offset of the dynamic array, its (tag, value) entries up to DT_NULL, file offset of the dynamic string
    table) of a little-endian ELF64 shared object."""
    import struct

    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, "not a little-endian ELF64 file"
    phoff, = struct.unpack_from("<Q", data, 0x20)
    phentsize, phnum = struct.unpack_from("<HH", data, 0x36)
    phdrs = [struct.unpack_from("<IIQQQQQQ", data, phoff + i * phentsize) for i in range(phnum)]
    dyn_off = next(ph[2] for ph in phdrs if ph[0] == 2)  # PT_DYNAMIC
    entries = []
    while True:
        tag, val = struct.unpack_from("<qQ", data, dyn_off + 16 * len(entries))
        if tag == 0:  # DT_NULL
            break
        entries.append((tag, val))
    strtab = next(v for t, v in entries if t == 5)  # DT_STRTAB (an address: mapped to its file offset)
    strtab_off = next(ph[2] + strtab - ph[3] for ph in phdrs if ph[0] == 1 and ph[3] <= strtab < ph[3] + ph[5])
    return dyn_off, entries, strtab_off


def _needed(path):
    """The DT_NEEDED entries of a shared object."""
    with open(path, "rb") as f:
        data = f.read()
    _, entries, strtab_off = _dynamic(data)
    return [data[strtab_off + v:data.index(b"\0", strtab_off + v)].decode() for t, v in entries if t == 1]


def _drop_needed(path, basename):
    """The bytes of a shared object with the DT_NEEDED entries whose file name is `basename` removed (the entries
    after them move up; the array keeps its length, ending in DT_NULL)."""
    import struct

    with open(path, "rb") as f:
        data = bytearray(f.read())
    dyn_off, entries, strtab_off = _dynamic(data)

    def name(v):
        return data[strtab_off + v:data.index(b"\0", strtab_off + v)].decode()

    kept = [(t, v) for t, v in entries if not (t == 1 and os.path.basename(name(v)) == basename)]
    for i in range(len(entries) + 1):
        struct.pack_into("<qQ", data, dyn_off + 16 * i, *(kept[i] if i < len(kept) else (0, 0)))
    return bytes(data)


def load_ref():
    """Import the prebuilt module (does not need /root/reference)."""
    import importlib.util

    import torch  # noqa: F401  (the extension links libtorch)

    p = built_path()
    if not os.path.exists(p):
        return None
    spec = importlib.util.spec_from_file_location(NAME, p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    ok = build(verbose="-v" in sys.argv)
    print("[oracle/_ref]", "ok" if ok else "not built")
    okb = build_option_b(verbose="-v" in sys.argv)
    print("[oracle/_ref] option-B module", "ok" if okb else "not built")
    sys.exit(0 if ok else 1)
