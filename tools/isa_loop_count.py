#!/usr/bin/env python3
"""Static instruction counts of an env kernel's fused-loop copy, by source function.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -gline-tables-only --cuda-device-only -S \\
          -I include -I marl-coverage_amd/csrc -o c2.s marl-coverage_amd/csrc/mc_env_inst_c2.hip
    tools/isa_loop_count.py c2.s marl-coverage_amd/csrc/mc_env_step.h ShapeC2BV

Takes the kernel whose mangled name holds the third argument, skips everything
before the first instruction attributed to env_kernel's step loop (so step 0's
straight-line copy is left out) and counts the rest by the function of
mc_env_step.h that the instruction's .loc line lies in (-gline-tables-only names
the innermost inlined function's line).  Classes: VALU, SALU, SMEM, LDS, VMEM,
s_waitcnt, v_writelane / v_readlane (SGPR spill traffic, also in VALU).

These are totals over EVERY path of the loop copy -- the in-step reset, the
sentinel and the obs-only path included -- not the hot path: use them to see
where a change moved instructions, and the SQ counters of tools/prof_config.py
--sq for what a step issues.

    tools/isa_loop_count.py --blocks c2.s marl-coverage_amd/csrc/mc_env_step.h ShapeC2BV

lists the loop copy's basic blocks instead, in layout order: the block's label
(or +n for the fall-through block after a conditional branch), its counts per
class, the functions its instructions come from, and where it ends -- the
branch's mnemonic and target, or "falls through".  A path through the step is
then a sum of rows: follow the targets.  Instruction classes only.
Needs no GPU."""
import collections
import re
import sys


def function_starts(header):
    starts = []
    for i, line in enumerate(open(header), 1):
        m = re.match(r"(?:__device__ __forceinline__|__global__).*?\b(\w+)\(", line)
        if m and not line.startswith(" "):
            starts.append((i, m.group(1)))
        if re.match(r"\s+auto place = ", line):
            starts.append((i, "place"))
        if re.match(r"\s+for \(int k = 1; k < num_steps", line):
            starts.append((i, "loop_body"))
    return sorted(starts)


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        return "VMEM"
    return "other"


def list_blocks(lines, fid, loop, fn, cols):
    """The loop copy's basic blocks in layout order (--blocks)."""
    cur, in_loop = ("?", 0), False
    rows, blk = [], None

    def start(label):
        return {"label": label, "n": collections.Counter(), "fns": [], "end": "falls through"}

    nfall = 0
    for line in lines:
        t = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            cur = (m.group(1), int(m.group(2)))
            if cur[0] == fid and loop <= cur[1] < loop + 30:
                in_loop = True
            continue
        if not in_loop:
            continue
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            if blk is not None:
                rows.append(blk)
            blk = start(m.group(1))
            continue
        if not t or t[0] in ".;" or t.endswith(":"):
            continue
        if blk is None:
            blk = start("(loop entry)")
        op = t.split()[0]
        blk["n"][classify(op)] += 1
        if op in ("v_writelane_b32", "v_readlane_b32"):
            blk["n"][op[2:-4]] += 1
        name = fn(cur[1]) if cur[0] == fid else "other files"
        if name not in blk["fns"]:
            blk["fns"].append(name)
        if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_setpc_b64"):
            target = t.split()[1] if len(t.split()) > 1 else ""
            blk["end"] = (op + " " + target).strip()
            rows.append(blk)
            nfall += 1
            blk = start("+%d" % nfall) if op.startswith("s_cbranch") else None
    if blk is not None:
        rows.append(blk)
    print("%-14s" % "block" + "".join("%6s" % c[:5] for c in cols) + "  ends with / from")
    total = collections.Counter()
    for b in rows:
        if not b["fns"]:  # an empty fall-through stub
            continue
        print("%-14s" % b["label"] + "".join("%6d" % b["n"][k] for k in cols) + "  " + b["end"] + "  [" +
              ", ".join(b["fns"]) + "]")
        total += b["n"]
    print("%-14s" % "TOTAL" + "".join("%6d" % total[k] for k in cols))


def main():
    args = sys.argv[1:]
    blocks = "--blocks" in args
    if blocks:
        args.remove("--blocks")
    asm, header, kernel = args[:3]
    starts = function_starts(header)
    loop = next((st for st, n in starts if n == "loop_body"), 0)

    def fn(line):
        name = "?"
        for st, n in starts:
            if st > line:
                break
            name = n
        return name

    text = open(asm).read()
    fid = None
    for m in re.finditer(r"\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?", text):
        if (m.group(3) or m.group(2)).endswith("mc_env_step.h"):
            fid = m.group(1)
    lines = text.split("\n")
    beg = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*env_kernel\w*:", l) and kernel in l), None)
    if beg is None:
        sys.exit(f"no env_kernel with {kernel} in {asm}")
    end = next(i for i in range(beg, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    cur, in_loop = ("?", 0), False
    agg = collections.defaultdict(collections.Counter)
    cols = ["VALU", "SALU", "SMEM", "LDS", "VMEM", "wait", "writelane", "readlane"]
    if blocks:
        return list_blocks(lines[beg:end], fid, loop, fn, cols)
    for line in lines[beg:end]:
        t = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            cur = (m.group(1), int(m.group(2)))
            if cur[0] == fid and loop <= cur[1] < loop + 30:
                in_loop = True
            continue
        if not t or t[0] in ".;" or t.endswith(":") or not in_loop:
            continue
        op = t.split()[0]
        name = fn(cur[1]) if cur[0] == fid else "other files"
        agg[name][classify(op)] += 1
        if op in ("v_writelane_b32", "v_readlane_b32"):
            agg[name][op[2:-4]] += 1
    print("%-22s" % "function" + "".join("%10s" % c for c in cols))
    total = collections.Counter()
    for name, c in sorted(agg.items(), key=lambda kv: -kv[1]["VALU"]):
        print("%-22s" % name + "".join("%10d" % c[k] for k in cols))
        total += c
    print("%-22s" % "TOTAL" + "".join("%10d" % total[k] for k in cols))


if __name__ == "__main__":
    main()
