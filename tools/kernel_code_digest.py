"""Digest of every kernel of one gfx950 code object: `symbol sha256(machine code) sha256(kernel descriptor)`, sorted by symbol.

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -c adam_score.hip -o adam_score.co
    python tools/kernel_code_digest.py adam_score.co > adam_score.digest

Two builds whose digests are equal hold the same kernels with the same instructions, registers and launch metadata,
whatever order the compiler emitted them in.  (The order follows the order in which the host code first names each
instantiation, so a change to a launcher permutes the assembly text and renumbers its labels without touching a kernel.)
A function's bytes do not depend on where it lies: branches are relative, and the step kernels reference no other section.
"""
import hashlib
import os
import subprocess
import sys

READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")


def sections(path):
    """name -> (address, file offset, size) from `llvm-readelf -S`."""
    out = subprocess.run([READELF, "-S", "-W", path], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        parts = line.replace("[", " ").replace("]", " ").split()
        if len(parts) >= 6 and parts[0].isdigit() and parts[1].startswith("."):
            table[parts[1]] = (int(parts[3], 16), int(parts[4], 16), int(parts[5], 16))
    return table


def symbols(path):
    """(name, address, size, type) from `llvm-readelf -s`."""
    out = subprocess.run([READELF, "-s", "-W", path], check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 8 and parts[0].rstrip(":").isdigit() and parts[3] in ("FUNC", "OBJECT"):
            yield parts[7], int(parts[1], 16), int(parts[2]), parts[3]


def main(path):
    data = open(path, "rb").read()
    secs = sections(path)

    def content(addr, size):
        for a, off, sz in secs.values():
            if a <= addr and addr + size <= a + sz:
                return data[off + addr - a: off + addr - a + size]
        raise SystemExit(f"no section holds {addr:#x}+{size}")

    code, desc = {}, {}
    for name, addr, size, kind in symbols(path):
        if kind == "FUNC":
            code[name] = hashlib.sha256(content(addr, size)).hexdigest()
        elif name.endswith(".kd"):
            kd = content(addr, size)   # bytes 16..23 are the distance from the descriptor to its code: position, not content
            desc[name[:-3]] = hashlib.sha256(kd[:16] + kd[24:]).hexdigest()
    for name in sorted(desc):
        print(name, code[name], desc[name])
    print(f"# {len(desc)} kernels", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1])
