#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds instruction by instruction.

    tools/isa_diff.py --a OLD.o [...] --b NEW.o [...] [--map NEW_SHAPE=OLD_SHAPE ...]

Each side is one or more objects or shared libraries.  From every file the
gfx950 code objects are taken out of the .hip_fatbin section (the offload
bundles are split by hand) and disassembled with llvm-objdump; addresses,
encodings, symbol names and the fill after a kernel's last instruction are
dropped.  Kernels are matched by their demangled name; env_kernel
instantiations by <NT, EPW, word> and shape, a --map entry renaming side b's
shape to side a's (e.g. 'ShapeC2=Shape<4, 10, 21, 2, 10, 8, 3, 0, 0, 0, 0, 0, 0>').
Prints per kernel whether the instruction streams are equal and the code-object
notes (VGPRs, SGPRs, spills, LDS, private segment) side by side; exit status 1
on any difference or unmatched kernel.  Needs no GPU."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
NOTES = ["vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
         "private_segment_fixed_size"]
# fill after a kernel ("...": llvm-objdump's run of zero words)
FILL = re.compile(r"\.\.\.$|s_nop 0$|s_code_end$|v_cndmask_b32_e32 v0, s0, v0$|\.long 0x00000000$")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    """The gfx950 code objects bundled in `path`, as files under tmp."""
    fb = os.path.join(tmp, "fatbin")
    if ".hip_fatbin" not in tool("llvm-readelf", "-S", path):
        return []  # host code only
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, path, os.path.join(tmp, "unused"))
    data, out = open(fb, "rb").read(), []
    for start in [m.start() for m in re.finditer(MAGIC, data)]:
        (n,), pos = struct.unpack_from("<Q", data, start + 24), start + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            triple, pos = data[pos + 24:pos + 24 + tlen], pos + 24 + tlen
            if triple.endswith(b"gfx950") and size:
                out.append(os.path.join(tmp, f"{os.path.basename(path)}.{len(out)}.co"))
                open(out[-1], "wb").write(data[start + off:start + off + size])
    return out


def kernels(co):
    """{demangled name: (instruction lines, notes)} of one code object."""
    plain = [l.split()[-1] for l in tool("llvm-objdump", "-t", co).splitlines() if " F .text" in l]
    pretty = [re.sub(r"^\.(protected|hidden) ", "", l.split(".text", 1)[1].split(None, 1)[1])
              for l in tool("llvm-objdump", "-t", "-C", co).splitlines() if " F .text" in l]
    demangled = dict(zip(plain, pretty))
    notes = {}
    for block in tool("llvm-readelf", "--notes", co).split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", block, re.M))
        notes[demangled[f["name"]]] = [int(f[k]) for k in NOTES]
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", "-C", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in notes else None
        elif cur is not None and line.startswith("\t"):
            cur.append(" ".join(line.split("//")[0].split()))
    for name, ins in out.items():
        while ins and FILL.match(ins[-1]):
            ins.pop()
        out[name] = (ins, notes[name])
    return out


def key(name, shapes):
    """An env_kernel's (NT, EPW, word, shape); any other kernel's own name."""
    m = re.match(r"void mc::env_kernel<(\d+), (\d+), (unsigned \w+), (.*)>\(mc::EnvArgs\)$", name)
    if not m:
        return name
    shape = m.group(4).replace("mc::", "").replace(" ", "")
    return "env_kernel<%s,%s,%s,%s>" % (m.group(1), m.group(2), m.group(3), shapes.get(shape, shape))


def side(paths, shapes, tmp):
    out = {}
    for p in paths:
        for co in code_objects(p, tmp):
            for name, v in kernels(co).items():
                k = key(name, shapes)
                if k in out:
                    sys.exit(f"{k}: more than once in {paths}")
                out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--map", action="append", default=[], metavar="B_SHAPE=A_SHAPE")
    args = ap.parse_args()
    shapes = {k.replace(" ", ""): v.replace(" ", "") for k, v in (m.split("=", 1) for m in args.map)}
    with tempfile.TemporaryDirectory() as tmp:
        a, b = side(args.a, {}, tmp), side(args.b, shapes, tmp)
    bad = 0
    print("%-74s %7s %6s  %s" % ("kernel", "insns", "code", "  ".join(n.replace("_count", "").replace("_fixed_size", "")
                                                                        for n in NOTES)))
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("%-74s only in %s" % (k, "a" if k in a else "b"))
            bad += 1
            continue
        (ia, na), (ib, nb) = a[k], b[k]
        same = ia == ib
        bad += (not same) + (na != nb)
        print("%-74s %7d %6s  %s" % (k, len(ib), "equal" if same else "DIFF",
                                     "  ".join(str(x) if x == y else f"{x}->{y}" for x, y in zip(na, nb))))
    print(f"{len(set(a) & set(b))} kernels on both sides, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
