#!/usr/bin/env python3
"""One SHA-256 per HIP source over its gfx950 device code: the .text disassembly, the metadata notes and the .rodata
dump (kernel descriptors: registers, LDS size, scratch), each with the file-name line stripped.  Two trees whose
digests agree ship the same instructions; the ELF itself is not hashed because two builds of one source already
differ in it (the __hip_cuid_* symbol).  Compiles the device side only, with the Makefile's flags; needs no GPU.
Usage: tools/device_code_digest.py [-DOPTION ...] sparch_amd/csrc/reccell.hip [more.hip ...]"""
import hashlib
import os
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = f"{ROCM}/lib/llvm/bin"
ARCH = "gfx950"
CXXFLAGS = [f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall",
            "-Wno-unused-function"]
FLAGS = {"cell.hip": ["-fno-slp-vectorize"]}      # as the Makefile's FLAGS_cell


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def digest(src, extra):
    with tempfile.TemporaryDirectory() as tmp:
        co, elf = f"{tmp}/x.co", f"{tmp}/x.elf"
        inc = os.path.join(os.path.dirname(os.path.abspath(src)), "../../include")      # the source's own tree
        run(f"{ROCM}/bin/hipcc", *CXXFLAGS, f"-I{inc}", *FLAGS.get(os.path.basename(src), []), *extra,
            "--cuda-device-only", "-c", src, "-o", co)
        run(f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={co}",
            f"--targets=hip-amdgcn-amd-amdhsa--{ARCH}", f"--output={elf}")
        text = (run(f"{LLVM}/llvm-objdump", "-d", elf) + run(f"{LLVM}/llvm-readelf", "--notes", elf)
                + run(f"{LLVM}/llvm-objdump", "-s", "-j", ".rodata", elf))
    lines = [ln for ln in text.splitlines() if elf not in ln]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


if __name__ == "__main__":
    extra = [a for a in sys.argv[1:] if a.startswith("-")]
    for src in (a for a in sys.argv[1:] if not a.startswith("-")):
        print(f"{digest(src, extra)}  {os.path.basename(src)}")
