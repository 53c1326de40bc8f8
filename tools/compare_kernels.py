"""Kernel-by-kernel comparison of the gfx950 code objects of two `hipcc --cuda-device-only -c` objects of one translation unit: the
set of kernel names, each kernel's code bytes (.text) and its 64-byte descriptor (.rodata).  For a host-only change of a unit both
must be equal; kernels present on one side only are listed.
usage: python tools/compare_kernels.py old.o new.o [--arch gfx950] [--llvm /opt/rocm/lib/llvm/bin]"""
import argparse
import os
import re
import subprocess
import tempfile


def code_object(obj, arch, llvm, tmp):
    """The unbundled ELF of `obj` (or `obj` itself when it already is one)."""
    with open(obj, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return obj
    out = os.path.join(tmp, os.path.basename(obj) + ".elf")
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets=hip-amdgcn-amd-amdhsa--{arch}",
                    f"--input={obj}", f"--output={out}"], check=True)
    return out


def kernels(elf, llvm):
    """{kernel name: (code bytes, descriptor bytes)}."""
    readelf = os.path.join(llvm, "llvm-readelf")
    sections = {}
    for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)",
                         subprocess.run([readelf, "-S", "-W", elf], capture_output=True, text=True, check=True).stdout):
        sections[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))       # name, address, file offset
    data = open(elf, "rb").read()
    func, desc = {}, {}
    for line in subprocess.run([readelf, "-s", "-W", elf], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) != 8 or not f[6].isdigit():
            continue
        value, size, kind, ndx, name = int(f[1], 16), int(f[2]), f[3], int(f[6]), f[7]
        _, addr, off = sections[ndx]
        blob = data[off + value - addr: off + value - addr + size]
        if kind == "FUNC":
            func[name] = blob
        elif kind == "OBJECT" and name.endswith(".kd"):
            # bytes 16 .. 23 are kernel_code_entry_byte_offset, the distance from the descriptor to the code: placement, not content
            desc[name[:-3]] = blob[:16] + blob[24:]
    return {n: (func[n], desc[n]) for n in desc if n in func}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default="/opt/rocm/lib/llvm/bin")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = (kernels(code_object(o, a.arch, a.llvm, tmp), a.llvm) for o in (a.old, a.new))
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0]
    for n in sorted(old.keys() - new.keys()):
        print("only in old:", demangle(n))
    for n in sorted(new.keys() - old.keys()):
        print("only in new:", demangle(n))
    differ = 0
    for n in sorted(old.keys() & new.keys()):
        code, kd = old[n][0] == new[n][0], old[n][1] == new[n][1]
        if not (code and kd):
            differ += 1
            print("differs:", demangle(n), "" if code else f"code ({len(old[n][0])} -> {len(new[n][0])} bytes)", "" if kd else "descriptor")
    print(f"kernels: {len(old)} old, {len(new)} new, {len(old.keys() & new.keys())} in both, {differ} of those differ")


main()
