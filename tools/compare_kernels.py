"""Kernel-by-kernel comparison of the gfx950 code of two builds: the set of kernel names, each kernel's code bytes (.text) and its
64-byte descriptor (.rodata).  Each side is one or more objects -- `hipcc -c` objects as the Makefile builds them (the code object is
taken out of their .hip_fatbin section) or `hipcc --cuda-device-only -c` ones -- and the comparison is over the union of a side by
kernel name, so a kernel that moved from one translation unit to another is not a difference.  For a host-only change all must be
equal; kernels present on one side only are listed.  A kernel that several units of a side carry (a small one from a shared header)
is compared as the set of its distinct copies.
usage: python tools/compare_kernels.py old.o new.o
       python tools/compare_kernels.py --old old/*.o --new new/*.o        [--arch gfx950] [--llvm /opt/rocm/lib/llvm/bin]"""
import argparse
import os
import re
import subprocess
import tempfile


def code_object(obj, arch, llvm, tmp):
    """The gfx950 ELF of `obj`: `obj` itself when it is one, else unbundled from it or from the .hip_fatbin section of a host object."""
    run = lambda *cmd: subprocess.run(cmd, check=True, capture_output=True)
    out = os.path.join(tmp, f"{len(os.listdir(tmp))}_{os.path.basename(obj)}")
    with open(obj, "rb") as f:
        head = f.read(20)
    if head[:4] == b"\x7fELF":
        if head[18:20] == b"\xe0\x00":           # e_machine = EM_AMDGPU
            return obj
        sections = subprocess.run([os.path.join(llvm, "llvm-readelf"), "-S", "-W", obj], capture_output=True, text=True, check=True).stdout
        if ".hip_fatbin" not in sections:
            return None                          # a unit without device code
        run(os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={out}.fatbin", obj)
        obj = out + ".fatbin"
    run(os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets=hip-amdgcn-amd-amdhsa--{arch}",
        f"--input={obj}", f"--output={out}.elf")
    return out + ".elf"


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


def side(objs, arch, llvm, tmp, label):
    """{kernel name: the set of its distinct (code, descriptor) copies} over `objs`, with the per-object counts printed."""
    union = {}
    for o in objs:
        elf = code_object(o, arch, llvm, tmp)
        ks = kernels(elf, llvm) if elf else {}
        print(f"{label} {o}: {len(ks)} kernels")
        for n, k in ks.items():
            union.setdefault(n, set()).add(k)
    return union


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pair", nargs="*", help="old.o new.o")
    ap.add_argument("--old", nargs="+", default=[])
    ap.add_argument("--new", nargs="+", default=[])
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default="/opt/rocm/lib/llvm/bin")
    a = ap.parse_args()
    if a.pair and (a.old or a.new or len(a.pair) != 2) or not a.pair and not (a.old and a.new):
        ap.error("give either old.o new.o, or --old ... --new ...")
    if a.pair:
        a.old, a.new = a.pair[:1], a.pair[1:]
    with tempfile.TemporaryDirectory() as tmp:
        old, new = (side(objs, a.arch, a.llvm, tmp, label) for objs, label in ((a.old, "old"), (a.new, "new")))
    demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0]
    for n in sorted(old.keys() - new.keys()):
        print("only in old:", demangle(n))
    for n in sorted(new.keys() - old.keys()):
        print("only in new:", demangle(n))
    differ = 0
    for n in sorted(old.keys() & new.keys()):
        if old[n] == new[n]:
            if len(old[n]) > 1:
                print(f"equal on both sides, in {len(old[n])} distinct copies (units built with different flags):", demangle(n))
            continue
        differ += 1
        (oc, ok), (nc, nk) = min(old[n] - new[n] or old[n]), min(new[n] - old[n] or new[n])
        print("differs:", demangle(n), "" if oc == nc else f"code ({len(oc)} -> {len(nc)} bytes)", "" if ok == nk else "descriptor")
    print(f"kernels: {len(old)} old, {len(new)} new, {len(old.keys() & new.keys())} in both, {differ} of those differ")


main()
