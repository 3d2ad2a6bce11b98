"""Time mc_frontier_actions (csrc/mc_dijkstra.hip's move sink,
``BatchCoverageEnv.frontier_actions``) against the dijkstra_input obs layer,
the same BFS kernels with the crop sink.

The C2 shape (4 agents, 128 x 128, 4096 envs), states taken 50 and 150 random
steps into the episode.  Two measurements:

1. the event-timed cost of one ``frontier_actions`` call: device events around
   windows of --calls calls after a warm-up, --reps repetitions per state;
2. in a separate ``rocprofv3 --kernel-trace --stats`` run of this tool's
   --workload mode (a fresh child process), the kernel times of the frontier
   call next to those of the dijkstra layer: a ``dijkstra_input=1`` handle
   forked to the same states rewrites its observation (a reset with an empty
   mask: the env kernel and then the layer's BFS kernels), and only its BFS
   kernels are counted.  --reps calls of each per state, alternating.

The new kernels run the same search and store less, so the condition is: the
frontier kernels' summed time (median over the repetitions) is no more than the
dijkstra layer's plus the spread of the repetitions (the larger max - min of
the two).  Prints one JSON line and writes it, with a README, into --out
(default profiles/r18/frontier).

The refactoring that gave the BFS kernels their sinks moved the obs kernels'
ISA (tools/isa_diff.py), so --out also holds c2_dijkstra_ab.json: bench.py
--config c2_dijkstra lines of the parent commit and of this tree, alternated
in one GPU call.  When the file is there, the README renders it as section 3.

    python tools/frontier_bench.py [--out DIR] [--calls 20] [--reps 7] [--envs 4096]
"""
import argparse
import collections
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = dict(numrobot=4, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
            dist_reward=0, train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0,
            allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
            sensor_config={"num_lasers": 21, "range": 10})
STATES = (50, 150)  # random steps into the episode
FRONTIER_KERNELS = ("frontier_window_kernel", "frontier_kernel", "frontier_big_kernel")
DIJKSTRA_KERNELS = ("dijkstra_window_kernel", "dijkstra_kernel", "dijkstra_big_kernel")


def make_envs(envs, with_layer):
    """The plain C2 env and, with_layer, a dijkstra_input=1 handle of the same pool to fork to."""
    import marlcov
    gen = dict(width=128, length=128, prob_obst=0.1, seed=1000)
    env = marlcov.BatchCoverageEnv(BASE, envs, gen=gen, seed=1, auto_reset=True)
    env.reset()
    layer = None
    if with_layer:  # (the same seeded pool; a fork copies each env's grid index with its state)
        layer = marlcov.BatchCoverageEnv(dict(BASE, dijkstra_input=1), envs, gen=gen, seed=1, auto_reset=False)
        layer.reset()
    return env, layer


def walk(env, t0, t1):
    for t in range(t0, t1):
        env.step(env.random_actions(7, t))


def window_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def timed(a):
    """Measurement 1: event-timed frontier_actions calls per state."""
    import torch
    env, _ = make_envs(a.envs, False)
    out = torch.empty((env.num_envs, env.num_agents), dtype=torch.uint8, device=env.device)
    res, t0 = {}, 0
    for steps in STATES:
        walk(env, t0, steps)
        t0 = steps
        _, dist, _ = env.frontier()
        for _ in range(3):
            env.frontier_actions(out=out)
        torch.cuda.synchronize()
        us = [window_us(torch, lambda: env.frontier_actions(out=out), a.calls) for _ in range(a.reps)]
        d = dist.flatten().cpu()
        res[str(steps)] = dict(call_us=us, call_us_median=sorted(us)[a.reps // 2], call_us_spread=max(us) - min(us),
                               dist_max=int(d.max()), dist_past_window=int((d > 24).sum()),
                               dist_none=int((d < 0).sum()))
    env.check()
    return dict(variant=env.frontier_variant(), states=res)


def workload(a):
    """Measurement 2's child: per state, --reps times one frontier call and one rewrite of the
    dijkstra layer on the forked handle.  Prints the dispatch plan the parent checks."""
    import torch
    env, layer = make_envs(a.envs, True)
    out = torch.empty((env.num_envs, env.num_agents), dtype=torch.uint8, device=env.device)
    same = torch.arange(env.num_envs, dtype=torch.int32, device=env.device)
    none = torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device)
    env.frontier_actions(out=out)  # setup, outside the counted calls (its kernels are dropped below)
    torch.cuda.synchronize()
    t0 = 0
    for steps in STATES:
        walk(env, t0, steps)
        t0 = steps
        layer.fork(same, env)
        for _ in range(a.reps):
            env.frontier_actions(out=out)
            layer.reset(env_mask=none)
            torch.cuda.synchronize()
    env.check()
    layer.check()
    print(json.dumps(dict(frontier_variant=env.frontier_variant(), dijkstra_variant=layer.dijkstra_variant())))


def kernel_times(path):
    """[(short kernel name, us)] of every dispatch in order."""
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1].split()[-1].replace(".kd", "")
        out.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    return out


def summarise(times, reps):
    """Per state and side: the summed BFS-kernel time of each repetition, and each kernel's own."""
    per = collections.defaultdict(list)
    for name, us in times:
        per[name].append(us)
    res = {}
    for side, names in (("frontier", FRONTIER_KERNELS), ("dijkstra", DIJKSTRA_KERNELS)):
        used = [n for n in names if per.get(n)]
        # the frontier side's first call (the setup call before the states) is not counted
        skip = 1 if side == "frontier" else 0
        # the dijkstra handle also ran its layer at its own resets (sibling) before the states: count from the end
        for n in used:
            if len(per[n]) < len(STATES) * reps + skip:
                raise SystemExit(f"frontier_bench: {n} has {len(per[n])} dispatches, expected at least "
                                 f"{len(STATES) * reps + skip}")
            per[n] = per[n][-len(STATES) * reps:]
        for k, steps in enumerate(STATES):
            sums = [sum(per[n][k * reps + r] for n in used) for r in range(reps)]
            res.setdefault(str(steps), {})[side] = dict(
                kernels={n: per[n][k * reps:(k + 1) * reps] for n in used}, sum_us=sums,
                sum_us_median=sorted(sums)[reps // 2], sum_us_spread=max(sums) - min(sums))
    for steps, r in res.items():
        spread = max(r["frontier"]["sum_us_spread"], r["dijkstra"]["sum_us_spread"])
        r["spread_us"] = spread
        r["condition_holds"] = r["frontier"]["sum_us_median"] <= r["dijkstra"]["sum_us_median"] + spread
    return res


def traced(a):
    """Measurement 2: the --workload child under rocprofv3 (its own run, kernel trace only)."""
    tdir = os.path.join(a.out, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--workload", "--envs", str(a.envs), "--reps", str(a.reps)]
    os.environ.setdefault("TMPDIR", "/tmp")
    with open(os.path.join(a.out, "trace.log"), "w") as f:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd, stdout=f, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise SystemExit(f"frontier_bench: the traced run failed ({r.returncode}), see {a.out}/trace.log")
    return summarise(kernel_times(tdir), a.reps)


def readme(res):
    rng = lambda v: f"{min(v):.1f}-{max(v):.1f}"  # noqa: E731
    rows1 = [f"| {s} | {r['dist_max']} | {r['dist_past_window']} | {r['dist_none']} | {rng(r['call_us'])} | "
             f"{r['call_us_median']:.1f} | {r['call_us_spread']:.1f} |" for s, r in res["timed"]["states"].items()]
    rows2, kern = [], []
    for s, r in res["traced"].items():
        f, d = r["frontier"], r["dijkstra"]
        rows2.append(f"| {s} | {rng(f['sum_us'])} | {f['sum_us_median']:.1f} | {rng(d['sum_us'])} | "
                     f"{d['sum_us_median']:.1f} | {r['spread_us']:.1f} | {'holds' if r['condition_holds'] else 'FAILS'} |")
        for side in (f, d):
            for n, v in side["kernels"].items():
                kern.append(f"| {s} | {n} | {rng(v)} | {sorted(v)[len(v) // 2]:.1f} |")
    ok = all(r["condition_holds"] for r in res["traced"].values())
    return "\n".join([
        "# Nearest-frontier moves: mc_frontier_actions against the dijkstra_input layer's kernels",
        "",
        f"`tools/frontier_bench.py`, C2 shape ({res['envs']} envs, 4 agents, 128 x 128, lidar 21 beams range 10), states",
        f"taken {' and '.join(str(s) for s in STATES)} random steps into the episode; kernel choice `{res['timed']['variant']}`.",
        "Times in microseconds; ranges are min-max over the repetitions, spread = max - min.",
        "",
        "## 1. One `frontier_actions` call, event-timed",
        "",
        f"Device events around windows of {res['calls']} calls after a warm-up, {res['reps']} repetitions per state.",
        "`dist max`: the farthest nearest-unexplored cell of the 16,384 agents; `past window`: agents whose target is",
        "farther than the window kernel's 24 exact layers (solved by the full-map kernel); `none`: no reachable target.",
        "",
        "| state (steps) | dist max | past window | none | call us | median | spread |",
        "|---|---|---|---|---|---|---|",
        *rows1,
        "",
        "## 2. Kernel times, `rocprofv3 --kernel-trace --stats` (a run of its own)",
        "",
        f"Per state, {res['reps']} times alternating: one frontier call on the plain handle, and one rewrite of the",
        "observation (a reset with an empty mask) on a `dijkstra_input=1` handle forked to the same state, of which",
        "only the layer's BFS kernels are counted.  Sum = window kernel + full-map kernel of one call.",
        "",
        "| state (steps) | frontier sum us | median | dijkstra layer sum us | median | spread | condition |",
        "|---|---|---|---|---|---|---|",
        *rows2,
        "",
        "Condition: the frontier kernels' median sum is no more than the dijkstra layer's plus the spread of the",
        "repetitions (the larger of the two sides' max - min). " + ("It holds for both states." if ok else "It FAILS."),
        "",
        "| state (steps) | kernel | us | median |",
        "|---|---|---|---|",
        *kern,
        "",
        "Raw numbers: `frontier_bench.json`.",
        "",
        *ab_section(res.get("c2_dijkstra_ab")),
    ])


def ab_section(ab):
    """Section 3 from c2_dijkstra_ab.json: {"command": ..., "parent": [...], "branch": [...]}, each entry
    {"env_steps_per_s", "kernel_us"} of one bench.py line."""
    if not ab:
        return []
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else sum(sorted(v)[len(v) // 2 - 1:len(v) // 2 + 1]) / 2  # noqa: E731
    rows, stat = [], {}
    for side in ("parent", "branch"):
        rate = [r["env_steps_per_s"] / 1e6 for r in ab[side]]
        us = [r["kernel_us"] for r in ab[side]]
        stat[side] = (med(us), max(us) - min(us))
        rows.append(f"| {side} | {', '.join(f'{v:.2f}' for v in rate)} | {med(rate):.2f} | "
                    f"{', '.join(f'{v:.2f}' for v in us)} | {med(us):.2f} | {max(us) - min(us):.2f} |")
    gap = abs(stat["parent"][0] - stat["branch"][0])
    spread = max(stat["parent"][1], stat["branch"][1])
    return [
        "## 3. The `dijkstra_input` layer itself, parent against this tree",
        "",
        "The obs kernels' bodies became inlined templates; `tools/isa_diff.py` reports the same instruction counts,",
        "registers, LDS and spills but differences in operand order and scheduling.  " + ab["command"] + ";",
        "`kernel us` is the line's `roofline.kernel_us` (every kernel of a step, HIP events around the 200 steps).",
        "",
        "| side | M env-steps/s, in run order | median | kernel us per step | median | spread |",
        "|---|---|---|---|---|---|",
        *rows,
        "",
        f"The medians differ by {gap:.2f} us, the repetitions spread over {spread:.2f} us: "
        + ("the two agree within the spread." if gap <= spread else "the two DIFFER by more than the spread."),
        "",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "frontier"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--limit", type=int, default=240, help="time limit of the traced run, seconds")
    ap.add_argument("--workload", action="store_true", help="the traced run's child: no timing, no files")
    ap.add_argument("--render", action="store_true", help="no device: rewrite the README from --out's JSON files")
    a = ap.parse_args()
    if a.render:
        res = json.load(open(os.path.join(a.out, "frontier_bench.json")))
        ab = os.path.join(a.out, "c2_dijkstra_ab.json")
        if os.path.exists(ab):
            res["c2_dijkstra_ab"] = json.load(open(ab))
        with open(os.path.join(a.out, "README.md"), "w") as f:
            f.write(readme(res))
        return None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frontier_bench: no HIP device")
    if a.workload:
        return workload(a)
    os.makedirs(a.out, exist_ok=True)
    res = dict(tool="tools/frontier_bench.py", calls=a.calls, reps=a.reps, envs=a.envs, states=list(STATES))
    res["timed"] = timed(a)
    res["traced"] = traced(a)
    ab = os.path.join(a.out, "c2_dijkstra_ab.json")
    if os.path.exists(ab):
        res["c2_dijkstra_ab"] = json.load(open(ab))
    with open(os.path.join(a.out, "frontier_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
