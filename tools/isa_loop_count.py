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
--sq for what a step issues.  Needs no GPU."""
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


def main():
    asm, header, kernel = sys.argv[1:4]
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
    cols = ["VALU", "SALU", "SMEM", "LDS", "VMEM", "wait", "writelane", "readlane"]
    print("%-22s" % "function" + "".join("%10s" % c for c in cols))
    total = collections.Counter()
    for name, c in sorted(agg.items(), key=lambda kv: -kv[1]["VALU"]):
        print("%-22s" % name + "".join("%10d" % c[k] for k in cols))
        total += c
    print("%-22s" % "TOTAL" + "".join("%10d" % total[k] for k in cols))


if __name__ == "__main__":
    main()
