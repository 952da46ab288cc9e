#!/usr/bin/env python3
"""Device code of two builds, compared without a GPU.

    scripts/device_code_hashes.py BUILD_DIR_A BUILD_DIR_B > profiles/NAME.md

For every object of either build directory that carries a gfx950 code object with a .text section
(extracted as scripts/kernel_regs.py does), the sha256 (16 hex) of its .text, .rodata and .note
sections. Sections, not whole files: a code object's symbol table carries the source path, so two
checkouts of identical source differ as files. For the same reason a kernel descriptor's code
entry (in .rodata, relative to the descriptor itself) is hashed as an offset into .text: the
translation unit's id symbol (__hip_cuid_<hex>, a hash of the source path, printed without leading
zeros) sits in .dynstr before .rodata, and a name one character shorter moves every descriptor by
an alignment step. Exit status 1 if a kernel object is missing from one build or any section differs.
"""
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_regs import LLVM, code_objects  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


def rebase_code_entries(co: str, rodata: bytes) -> bytes:
    """.rodata with each kernel descriptor's kernel_code_entry_byte_offset (8 bytes at +16, relative
    to the descriptor) replaced by the entry's offset in .text."""
    vma = {}
    for line in subprocess.run([f"{LLVM}/llvm-objdump", "-h", co], capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) >= 4 and f[1] in (".rodata", ".text"):
            vma[f[1]] = int(f[3], 16)
    out = bytearray(rodata)
    for line in subprocess.run([f"{LLVM}/llvm-objdump", "-t", co], capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        if len(f) >= 5 and f[-1].endswith(".kd") and ".rodata" in f:
            at = int(f[0], 16) - vma[".rodata"] + 16
            entry = int(f[0], 16) + int.from_bytes(out[at:at + 8], "little", signed=True) - vma[".text"]
            out[at:at + 8] = entry.to_bytes(8, "little", signed=True)
    return bytes(out)


def section_hashes(co: str, tmp: str) -> dict:
    out = {}
    for sec in SECTIONS:
        dump = os.path.join(tmp, "section.bin")
        if os.path.exists(dump):
            os.remove(dump)
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section={sec}={dump}", co, os.path.join(tmp, "y.o")],
                       capture_output=True)
        data = open(dump, "rb").read() if os.path.exists(dump) else b""
        if sec == ".rodata" and data:
            data = rebase_code_entries(co, data)
        out[sec] = f"{hashlib.sha256(data).hexdigest()[:16]} ({len(data)} B)" if data else "-"
    return out


def build_hashes(objdir: str) -> dict:
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(objdir)):
            if not name.endswith(".o"):
                continue
            for co in code_objects(os.path.join(objdir, name), tmp):
                h = section_hashes(co, tmp)
                if h[".text"] != "-":
                    res[name] = h
    return res


def main() -> int:
    a, b = build_hashes(sys.argv[1]), build_hashes(sys.argv[2])
    bad = 0
    print("| object | section | A | B | equal |")
    print("|---|---|---|---|---|")
    for name in sorted(set(a) | set(b)):
        for sec in SECTIONS:
            x, y = a.get(name, {}).get(sec, "missing"), b.get(name, {}).get(sec, "missing")
            bad += x != y
            print(f"| {name} | {sec} | {x} | {y} | {'yes' if x == y else 'NO'} |")
    print(f"\n{len(set(a) | set(b))} kernel objects, {bad} differing sections")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
