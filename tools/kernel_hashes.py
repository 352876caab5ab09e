#!/usr/bin/env python3
"""One line per kernel of a device-only gfx950 code object: the demangled name, the sha256 of its
machine code (the symbol's st_value .. st_value + st_size range of .text) and its resource figures
from the metadata note.  Two trees' outputs are compared with diff: a refactor of the hand-scheduled
files that moved nothing leaves every line of a surviving kernel as it was.  The .kd descriptor is
not hashed (its entry offset moves with the layout).  A kernel that addresses a __device__ global
(the MCS_STAMPS probe builds' counters) holds a pc-relative displacement to its GOT slot, which
also moves when kernels come or go: link with -Xoffload-linker --emit-relocs and every field that
.rela.text names is zeroed before hashing (the line then ends with their count), so what is
compared is the code and not where the linker put it.

    hipcc <the Makefile's flags for the file> --offload-device-only --no-gpu-bundle-output \
        -Xoffload-linker --emit-relocs -c -o fifo_asm.co csrc/mcs_fifo_asm.hip
    tools/kernel_hashes.py fifo_asm.co
"""
import hashlib
import os
import re
import subprocess
import sys

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")
SYM = re.compile(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+\d+\s+(.*)$")
RELOC = re.compile(r"^([0-9a-f]{16})\s+[0-9a-f]{16}\s+(R_AMDGPU_\w+)")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def readelf(*args):
    return subprocess.run([READELF, "-W", *args], check=True, capture_output=True, text=True).stdout


def main(path):
    text = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", readelf("-S", path))
    addr, off, size = (int(g, 16) for g in text.groups())
    blob = bytearray(open(path, "rb").read())
    # relocated fields of .text (present only when linked with --emit-relocs): zeroed
    masked, in_text = [], False
    for line in readelf("-r", path).splitlines():
        if line.startswith("Relocation section"):
            in_text = "'.rela.text'" in line
        m = RELOC.match(line)
        if m and in_text:
            at, n = int(m.group(1), 16), 8 if m.group(2).endswith("64") else 4
            blob[off + at - addr : off + at - addr + n] = bytes(n)
            masked.append(at)
    # the metadata note: one entry per kernel, keyed by its mangled name
    figures, cur = {}, None
    for line in readelf("--notes", path).splitlines():
        if line.startswith("  - "):
            cur = {}
        m = re.match(r"(?:  - |    )\.(\w+):\s+(\S+)\s*$", line)  # (an entry's own keys, not its args')
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if "name" in cur:
                figures[cur["name"]] = cur
    mangled = [m.groups() for m in map(SYM.match, readelf("-s", path).splitlines()) if m]
    pretty = [m.group(4) for m in map(SYM.match, readelf("-s", "-C", path).splitlines()) if m]
    rows, seen = set(), set()
    for (value, n, kind, name), shown in zip(mangled, pretty):
        if kind != "FUNC" or name not in figures:
            continue  # a descriptor, a global or a device function, not a kernel
        lo, hi = int(value, 16), int(value, 16) + int(n)
        assert addr <= lo and hi <= addr + size, name
        f = figures[name]
        row = f"{shown}  {hashlib.sha256(blob[off + lo - addr : off + hi - addr]).hexdigest()}  {n} B  "
        row += " ".join(f"{k}={f[k]}" for k in FIGURES)
        fields = sum(lo <= at < hi for at in masked)
        rows.add(row + (f"  masked={fields}" if fields else ""))
        seen.add(name)
    # every kernel descriptor (.kd symbol) has its line: a kernel must not drop out unnoticed
    kd = {name[:-3] for _, _, kind, name in mangled if kind == "OBJECT" and name.endswith(".kd")}
    assert kd and kd == seen, f"kernels without a line: {sorted(kd - seen)}; lines without a .kd: {sorted(seen - kd)}"
    print("\n".join(sorted(rows)))


if __name__ == "__main__":
    main(sys.argv[1])
