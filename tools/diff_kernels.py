#!/usr/bin/env python3
"""Device code of two builds of the library, kernel by kernel (code objects only, no GPU needed).

For a refactoring that must leave the kernels alone: every gfx950 kernel of OLD.so and NEW.so is disassembled and
compared as text (addresses and encodings left out; branch targets are relative), and for the ones that differ the
instruction counts and the resource figures (VGPRs, SGPRs, spilled VGPRs, scratch bytes: check_spills.kernel_resources;
plus static LDS bytes) of both builds are printed.

    python tools/diff_kernels.py OLD.so NEW.so
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_spills import LLVM, demangle, kernel_resources  # noqa: E402


def kernels(lib):
    """{kernel name: (instruction lines, static LDS bytes)} for every gfx950 kernel in `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            path = os.path.join(tmp, f)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], check=True, capture_output=True,
                                   text=True).stdout
            lds = {}
            for blk in notes.split("- .agpr_count:")[1:]:
                name, size = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
                if name and size:
                    lds[name.group(1)] = int(size.group(1))
            asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path],
                                 check=True, capture_output=True, text=True).stdout
            name = None
            for line in asm.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
                if m:
                    name = m.group(1) if m.group(1) in lds else None
                    if name:
                        out[name] = ([], lds[name])
                elif name and line.strip():
                    text = re.sub(r"\s*//.*$", "", line).strip()
                    if text and not text.startswith("s_nop") and not text.startswith("s_code_end"):
                        out[name][0].append(text)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    res_old, res_new = kernel_resources(sys.argv[1]), kernel_resources(sys.argv[2])
    for what, names in (("only in OLD", sorted(set(old) - set(new))), ("only in NEW", sorted(set(new) - set(old)))):
        for name, pretty in zip(names, demangle(names)):
            print(f"{what}: {pretty[:160]}")
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k] or res_old[k] != res_new[k]]
    print(f"{len(both)} kernels in both, {len(both) - len(differ)} identical, {len(differ)} differ")
    for name, pretty in zip(differ, demangle(differ)):
        print(f"  {pretty[:160]}")
        print(f"      instructions {len(old[name][0])} -> {len(new[name][0])}; (VGPRs, SGPRs, spilled, scratch B) "
              f"{res_old[name]} -> {res_new[name]}; LDS B {old[name][1]} -> {new[name][1]}")
