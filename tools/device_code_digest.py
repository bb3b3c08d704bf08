#!/usr/bin/env python3
"""One SHA-256 per HIP source over its gfx950 device code: the .text disassembly, the metadata notes and the .rodata
dump (kernel descriptors: registers, LDS size, scratch), each with the file-name line stripped.  Two trees whose
digests agree ship the same instructions; the ELF itself is not hashed because two builds of one source already
differ in it (the __hip_cuid_* symbol).  Compiles the device side only, with the Makefile's flags; needs no GPU.
Usage: tools/device_code_digest.py [--per-symbol [--list]] [-DOPTION ...] sparch_amd/csrc/reccell.hip [more.hip ...]

--per-symbol: a digest that does not depend on the ORDER in which the compiler emits the kernels (host code that
names the same kernels in another order moves them).  Per kernel symbol: its disassembly with the absolute address
column stripped (branch targets are printed relative to the symbol; the pc-relative literal that forms the address of
a device global is replaced by the section and offset it reaches), its 64-byte kernel descriptor with the one
position-dependent field (kernel_code_entry_byte_offset, bytes 16-23) zeroed, and its entry of the metadata note.  The
printed value is the SHA-256 over the sorted (symbol, digest) pairs, followed by the number of kernels: equal values
mean the same set of symbols with identical instructions, descriptors and metadata.  --list prints the pairs too."""
import hashlib
import os
import re
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


def per_symbol(elf, tmp):
    """{kernel symbol: digest} of an unbundled code object."""
    symtab = [ln.split() for ln in run(f"{LLVM}/llvm-readelf", "-s", "-W", elf).splitlines()]
    sections = [(int(f[2], 16), int(f[4], 16), f[0]) for f in
                (ln.split("]", 1)[1].split() for ln in run(f"{LLVM}/llvm-readelf", "-S", "-W", elf).splitlines()
                 if re.match(r"\s*\[\s*[1-9]\d*\]", ln))]
    code, name, prev = {}, None, ""
    for ln in run(f"{LLVM}/llvm-objdump", "-d", elf).splitlines():
        m = re.match(r"^[0-9a-f]{16} <(.+)>:$", ln)
        if m:
            name = m.group(1)
            code[name] = []
        elif name and ln.strip():
            # the address of a device global (or of its GOT slot): s_getpc_b64 + a literal that depends on where the
            # kernel sits -> the section it reaches and the offset into it
            pc = re.match(r"\s*s_add_u32 (s\d+), \1, 0x([0-9a-f]+)\s+// ([0-9A-F]+): ", ln)
            if pc and prev.startswith("s_getpc_b64"):
                target = int(pc.group(3), 16) + int(pc.group(2), 16)
                base, sec = next((a, n) for a, size, n in sections if a <= target < a + size)
                ln = f"\ts_add_u32 {pc.group(1)}, {pc.group(1)}, pcrel({sec}+{target - base:#x})"
            prev = ln.strip()
            code[name].append(re.sub(r"// [0-9A-F]+: ", "// ", ln))
    rodata_addr = next(a for a, _, n in sections if n == ".rodata")
    run(f"{LLVM}/llvm-objcopy", "--dump-section", f".rodata={tmp}/rodata.bin", elf, f"{tmp}/unused.elf")
    rodata = open(f"{tmp}/rodata.bin", "rb").read()
    desc = {}
    for f in symtab:
        if len(f) == 8 and f[7].endswith(".kd"):
            off = int(f[1], 16) - rodata_addr
            kd = bytearray(rodata[off:off + 64])
            kd[16:24] = bytes(8)                            # kernel_code_entry_byte_offset: where the code sits
            desc[f[7][:-3]] = kd.hex()
    notes = run(f"{LLVM}/llvm-readelf", "--notes", elf)
    kernels = notes[notes.index("amdhsa.kernels:"):notes.index("amdhsa.target:")]
    meta = {}
    for block in re.split(r"\n  - ", kernels)[1:]:
        meta[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    assert set(code) == set(desc) == set(meta), "kernel symbols of .text, .rodata and the metadata note differ"
    return {k: hashlib.sha256("\n".join(code[k] + [desc[k], meta[k]]).encode()).hexdigest() for k in code}


def digest(src, extra, by_symbol=False, listing=False):
    with tempfile.TemporaryDirectory() as tmp:
        co, elf = f"{tmp}/x.co", f"{tmp}/x.elf"
        inc = os.path.join(os.path.dirname(os.path.abspath(src)), "../../include")      # the source's own tree
        run(f"{ROCM}/bin/hipcc", *CXXFLAGS, f"-I{inc}", *FLAGS.get(os.path.basename(src), []), *extra,
            "--cuda-device-only", "-c", src, "-o", co)
        run(f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={co}",
            f"--targets=hip-amdgcn-amd-amdhsa--{ARCH}", f"--output={elf}")
        if by_symbol:
            syms = sorted(per_symbol(elf, tmp).items())
            if listing:
                for k, d in syms:
                    print(f"    {d}  {k}", file=sys.stderr)
            return f"{hashlib.sha256(repr(syms).encode()).hexdigest()} {len(syms):4d} kernels"
        text = (run(f"{LLVM}/llvm-objdump", "-d", elf) + run(f"{LLVM}/llvm-readelf", "--notes", elf)
                + run(f"{LLVM}/llvm-objdump", "-s", "-j", ".rodata", elf))
    lines = [ln for ln in text.splitlines() if elf not in ln]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


if __name__ == "__main__":
    own = ("--per-symbol", "--list")
    extra = [a for a in sys.argv[1:] if a.startswith("-") and a not in own]
    for src in (a for a in sys.argv[1:] if not a.startswith("-")):
        print(f"{digest(src, extra, '--per-symbol' in sys.argv, '--list' in sys.argv)}  {os.path.basename(src)}")
