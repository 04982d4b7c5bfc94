"""VGPR / SGPR / scratch / LDS / occupancy / code length of every kernel in the device assembly of each
translation unit (make asm TU=...).
usage: python tools/kernel_regs.py [--reuse] [--only=PREFIX] <pkg dir> [<other pkg dir>]
  -> one line per kernel; with a second package directory, every figure that differs is flagged with the
     other's, the code length's change in per cent, and `=` marks a kernel whose instructions are identical (local
     labels compared without the function's number in the unit).
--reuse: read build/<unit>.s where it exists instead of assembling the unit again.
--only=PREFIX: the units whose name starts with PREFIX (dkg_env: the envelope buckets)."""
import os
import re
import subprocess
import sys

FIELDS = ("vgpr", "sgpr", "scratch", "lds", "occ", "len")


def regs(pkg, reuse, only):
    out = {}
    for f in sorted(os.listdir(os.path.join(pkg, "csrc"))):
        if not (f.endswith(".hip") and f.startswith(only)):
            continue
        tu = f[:-4]
        path = os.path.join(pkg, "build", tu + ".s")
        if not (reuse and os.path.exists(path)):
            subprocess.run(["make", "-s", "-C", pkg, "asm", f"TU={tu}"], check=True, capture_output=True)
        s = open(path).read()
        meta = {}
        for b in s.split("- .agpr_count")[1:]:
            n = re.search(r"\.name:\s+(\S+)", b).group(1)
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", b).group(1))  # noqa: E731
            meta[n] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"))
        # a kernel's text: from its label to its "; Kernel info:" comment block
        for mt in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^; Kernel info:\n(.*?)^; COMPUTE_PGM", s, re.M | re.S):
            n, body, info = mt.groups()
            if n not in meta:
                continue
            gi = lambda k: int(re.search(rf"^; {k}\s*[:=]\s*(\d+)", info, re.M).group(1))  # noqa: E731
            v, sg, sc, lds = meta[n]
            out[n] = dict(tu=tu, vgpr=v, sgpr=sg, scratch=sc, lds=lds, occ=gi("Occupancy"), len=gi("codeLenInByte"),
                          text=re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", body[: body.find(".section\t.rodata")]))
    return out


def short(n):
    """dkg::name<template arguments> of a mangled kernel name whose arguments are integers and bools; else n."""
    m = re.match(r"_ZN3dkg\d+([A-Za-z_0-9]+?)I((?:L[ib]\d+E)+)E", n)
    return n if m is None else m.group(1) + "<" + ", ".join(re.findall(r"L[ib](\d+)E", m.group(2))) + ">"


args = [x for x in sys.argv[1:] if not x.startswith("--")]
reuse = "--reuse" in sys.argv[1:]
only = next((x[7:] for x in sys.argv[1:] if x.startswith("--only=")), "")
a = regs(args[0], reuse, only)
b = regs(args[1], reuse, only) if len(args) > 1 else {}
print("vgpr sgpr scratch    lds occ     len  kernel")
same = worst = 0
for n in sorted(a):
    k, o = a[n], b.get(n)
    flag = "   <-- not in the other" if b and o is None else ""
    if o is not None:
        diff = [f"{f} {o[f]}" for f in FIELDS if o[f] != k[f]]
        if o["len"] != k["len"]:
            pct = 100.0 * (k["len"] - o["len"]) / o["len"]
            worst = max(worst, pct)
            diff.append(f"{pct:+.2f} %")
        ident = o["text"] == k["text"]
        same += ident
        flag = "  =" if ident else ("   <-- " + ", ".join(diff) if diff else "")
    print(f"{k['vgpr']:4d} {k['sgpr']:4d} {k['scratch']:7d} {k['lds']:6d} {k['occ']:3d} {k['len']:7d}  {short(n)}{flag}")
if b:
    gone = sorted(set(b) - set(a))
    print(f"# {len(a)} kernels, {same} with identical instructions, largest code growth {worst:+.2f} %"
          + (f", missing here: {gone}" if gone else ""))
