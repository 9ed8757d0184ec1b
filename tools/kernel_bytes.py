#!/usr/bin/env python3
"""Per-kernel machine-code fingerprints of liborx device units (no GPU needed):
  tools/kernel_bytes.py [-DDEFINE ...] -o OUT.txt UNIT.hip [UNIT.hip ...]
  tools/kernel_bytes.py --diff A.txt B.txt
Compiles each unit for gfx950 with the library's flags, device side only and unbundled, and writes
one line per kernel: unit, mangled name, code size, sha256 of the code bytes, sha256 of the 64-byte
kernel descriptor (<name>.kd, without its offset to the code). --diff pairs two such files by mangled name (the unit is not compared,
so a kernel that moved between units pairs with itself) and lists the kernels whose code or descriptor
differ and the ones on one side only; exit status 1 if there are any. Units are looked up under
oppositerenderer_amd/csrc unless the path exists as given."""
import argparse, hashlib, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oppositerenderer_amd", "csrc")
BIN = "/opt/rocm/llvm/bin/"
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-fast-math -fno-slp-vectorize -w").split()


def fingerprints(unit, defines, tmp):
    src = unit if os.path.exists(unit) else os.path.join(CSRC, unit)
    obj = os.path.join(tmp, "dev.elf")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "--offload-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj])
    sect = {}   # section index -> (address, file offset)
    for ln in subprocess.check_output([BIN + "llvm-readelf", "-S", "-W", obj], text=True).splitlines():
        f = ln.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[0].isdigit() and f[2] != "NULL":
            sect[int(f[0])] = (int(f[3], 16), int(f[4], 16))
    sym = {}    # name -> (type, bytes)
    data = open(obj, "rb").read()
    for ln in subprocess.check_output([BIN + "llvm-readelf", "-s", "-W", obj], text=True).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, size, (saddr, soff) = int(f[1], 16), int(f[2], 0), sect[int(f[6])]
            sym[f[7]] = (f[3], data[soff + addr - saddr: soff + addr - saddr + size])
    h = lambda b: hashlib.sha256(b).hexdigest()[:16]
    # bytes 16..23 of a descriptor are the distance from it to the code: where the kernel sits in its unit
    kd = lambda n: sym[n + ".kd"][1][:16] + bytes(8) + sym[n + ".kd"][1][24:]
    return [f"{os.path.basename(unit)} {n} {len(b)} {h(b)} {h(kd(n))}"
            for n, (t, b) in sorted(sym.items()) if t == "FUNC" and n + ".kd" in sym]


def diff(a, b):
    rd = lambda p: {f[1]: f for f in (ln.split() for ln in open(p)) if len(f) == 5}
    A, B = rd(a), rd(b)
    bad = 0
    for n in sorted(set(A) | set(B)):
        if n not in A or n not in B:
            print(f"only in {b if n not in A else a}: {n} ({(A.get(n) or B.get(n))[0]})")
        elif A[n][2:] != B[n][2:]:
            what = [w for w, i in (("size", 2), ("code", 3), ("descriptor", 4)) if A[n][i] != B[n][i]]
            print(f"differs ({', '.join(what)}): {n} ({A[n][0]} {A[n][2]} B -> {B[n][0]} {B[n][2]} B)")
        else:
            continue
        bad += 1
    print(f"{len(set(A) & set(B))} kernels on both sides, {bad} differ or are unpaired")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("-D", action="append", default=[], dest="defs", metavar="DEFINE")
    ap.add_argument("-o", dest="out")
    ap.add_argument("units", nargs="*")
    a = ap.parse_args()
    if a.diff:
        sys.exit(diff(*a.diff))
    with tempfile.TemporaryDirectory() as tmp:
        lines = [ln for u in a.units for ln in fingerprints(u, ["-D" + d for d in a.defs], tmp)]
    (open(a.out, "w") if a.out else sys.stdout).write("\n".join(lines) + "\n")
