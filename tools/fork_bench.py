"""Time mc_copy_envs / mc_sg_copy_envs (csrc/mc_fork.hip): a full-batch fork
from a sibling handle against the plain device-to-device copies a whole-batch
snapshot costs without it (mc_get_state of the maps, positions and per-env
scalars into preallocated buffers -- fewer bytes than the fork moves, which
favours the baseline).

Three workloads: the C2 shape (4 agents, 128 x 128, 4096 envs), the sg_c2
shape (SuperGridRL, same grid) and a C5-shaped handle of 256 envs (16 agents,
512 x 512, dist_reward: the top-cell cache travels too).  Device events around
windows of --calls calls after a warm-up, fork and baseline alternating in one
process, --reps repetitions each; a 1/8-batch fork (the other indices -1) is
recorded next to them.  Prints one JSON line and writes it, with a README,
into --out (default profiles/r10/fork).

    python tools/fork_bench.py [--out DIR] [--calls 50] [--reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK_GBS = 6290.0  # achievable float4 copy rate of one MI355X (79 % of the 8.0 TB/s HBM3E spec)

BASE = dict(maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30, dist_reward=0,
            train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0, allow_comm=0,
            map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
            sensor_config={"num_lasers": 21, "range": 10})
SG = dict(numrobot=4, train_maxsteps=1000, test_maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0,
          terminal_reward=30, senseradius=2, free_penalty=0.2, dist_reward=1, use_scanning=0)


def dec_workload(torch, numrobot, side, envs, dist):
    import marlcov
    from marlcov import _lib
    cfg = dict(BASE, numrobot=numrobot, dist_reward=dist)
    env = marlcov.BatchCoverageEnv(cfg, envs, gen=dict(width=side, length=side, prob_obst=0.1, seed=1000),
                                   seed=1, auto_reset=True)
    env.reset()
    for t in range(4):
        env.step(env.random_actions(7, t))
    sib = env.sibling(envs)
    lib, N, mw = env.lib, numrobot, int(env.layout.mask_words_per_agent)
    fields = [_lib.FIELD_POS, _lib.FIELD_FREE, _lib.FIELD_OBST, _lib.FIELD_VISITED, _lib.FIELD_MOVED,
              _lib.FIELD_DONE_THRESH, _lib.FIELD_FREE_COUNT, _lib.FIELD_VISITED_COUNT, _lib.FIELD_CURRSTEP,
              _lib.FIELD_ENV_GRID, _lib.FIELD_EPISODE]
    bufs = [env.get_state(f) for f in fields]
    sizes = [b.numel() * b.element_size() for b in bufs]
    # per env: the record, pos, free / obst / visited maps, the episode record
    per_env = 64 + 8 * N + 2 * N * mw * 8 + mw * 8 + 8 + 4
    if dist:
        cache = lib.mc_build_param(_lib.PARAM_DIST_CACHE_CELLS)
        per_env += N * 8 + N * 32  # DIST_MW, the PRE terms
        if not cfg["map_sharing"]:  # the top-cell cache is on
            per_env += N * (2 * cache * 4 + 32 + 64 * 4)  # cache cells, their d, header, strip maxima

    def fork(idx):
        return lib.mc_copy_envs(sib._h, env._h, idx.data_ptr(), env._stream())

    def baseline():
        st = env._stream()
        rc = 0
        for f, b, n in zip(fields, bufs, sizes):
            rc |= lib.mc_get_state(env._h, f, b.data_ptr(), n, st)
        return rc

    return dict(envs=envs, fork=fork, baseline=baseline, fork_bytes=2 * per_env * envs,
                baseline_bytes=2 * sum(sizes), baseline_calls=len(fields), keep=(env, sib, bufs))


def sg_workload(torch, side, envs):
    import marlcov
    from marlcov import _lib
    env = marlcov.BatchSuperGridEnv(SG, envs, gen=dict(width=side, length=side, prob_obst=0.1, seed=1000),
                                    seed=1, auto_reset=True, maxsteps=1000)
    env.reset()
    g = torch.Generator(device=env.device)
    g.manual_seed(0)
    for _ in range(4):
        env.step(torch.randint(0, 4, (envs, SG["numrobot"]), dtype=torch.uint8, device=env.device, generator=g))
    sib = env.sibling(envs)
    lib, N = env.lib, SG["numrobot"]
    fields = [_lib.SG_FIELD_POS, _lib.SG_FIELD_COVERED, _lib.SG_FIELD_OBST, _lib.SG_FIELD_COV_COUNT,
              _lib.SG_FIELD_CURRSTEP, _lib.SG_FIELD_DONE_THRESH, _lib.SG_FIELD_A_PREV, _lib.SG_FIELD_ENV_GRID,
              _lib.SG_FIELD_EPISODE]
    bufs = [env.get_state(f) for f in fields]
    sizes = [b.numel() * b.element_size() for b in bufs]
    mw, cells = side * env.row_words * 8, side * side
    # per env: two bitboards, the uint8 planes, the float32 distance layer, pos, the scalars
    per_env = 2 * mw + env.planes.shape[1] * cells + 4 * cells + 8 * N + 2 * 8 + 7 * 4 + 1

    def fork(idx):
        return lib.mc_sg_copy_envs(sib._h, env._h, idx.data_ptr(), env._stream())

    def baseline():
        st = env._stream()
        rc = 0
        for f, b, n in zip(fields, bufs, sizes):
            rc |= lib.mc_sg_get_state(env._h, f, b.data_ptr(), n, st)
        return rc

    # the registered state buffers are most of what the SuperGrid fork moves
    # and no state field: the same baseline plus plain copies of the two
    # buffers moves the fork's bytes (recorded next to the baseline proper)
    planes2, dist2 = torch.empty_like(env.planes), torch.empty_like(env.dist)

    def baseline_buffers():
        rc = baseline()
        planes2.copy_(env.planes)
        dist2.copy_(env.dist)
        return rc

    extra = 2 * (planes2.numel() + 4 * dist2.numel())
    return dict(envs=envs, fork=fork, baseline=baseline, fork_bytes=2 * per_env * envs,
                baseline_bytes=2 * sum(sizes), baseline_calls=len(fields), keep=(env, sib, bufs),
                baseline_buffers=baseline_buffers, baseline_buffers_bytes=2 * sum(sizes) + extra)


def window_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = 0
    for _ in range(calls):
        rc |= fn()
    e1.record()
    torch.cuda.synchronize()
    if rc:
        raise RuntimeError(f"a timed call failed ({rc})")
    return e0.elapsed_time(e1) * 1e3 / calls


def measure(torch, w, calls, reps, warmup=10):
    B = w["envs"]
    full = torch.arange(B, dtype=torch.int32, device="cuda")
    eighth = torch.where(full < B // 8, full, torch.full_like(full, -1))
    runs = {"fork": lambda: w["fork"](full), "baseline": w["baseline"], "fork_eighth": lambda: w["fork"](eighth)}
    if "baseline_buffers" in w:
        runs["baseline_buffers"] = w["baseline_buffers"]
    for fn in runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(reps):  # alternate in one process
        for k, fn in runs.items():
            us[k].append(window_us(torch, fn, calls))
    w["keep"][0].check()
    w["keep"][1].check()
    f, b = us["fork"], us["baseline"]
    spread = max(b) - min(b)
    med = sorted(f)[len(f) // 2]
    more = {}
    if "baseline_buffers" in w:
        more = dict(baseline_buffers_us=us["baseline_buffers"], baseline_buffers_bytes=w["baseline_buffers_bytes"])
    return dict(more, envs=B, fork_bytes=w["fork_bytes"], baseline_bytes=w["baseline_bytes"],
                baseline_calls=w["baseline_calls"], fork_us=f, baseline_us=b, fork_eighth_us=us["fork_eighth"],
                fork_gbs=w["fork_bytes"] / med / 1e3, fork_share_of_copy_peak=w["fork_bytes"] / med / 1e3 / COPY_PEAK_GBS,
                baseline_gbs=w["baseline_bytes"] / sorted(b)[len(b) // 2] / 1e3,
                # the fork's range does not lie above the baseline's by more than the baseline's spread
                condition_holds=max(f) <= max(b) + spread)


def readme(res):
    rows = []
    for name, r in res["workloads"].items():
        rows.append(f"| {name} | {r['envs']} | {r['fork_bytes'] / 1e6:.1f} | {min(r['fork_us']):.1f}-{max(r['fork_us']):.1f} | "
                    f"{r['fork_gbs']:.0f} ({100 * r['fork_share_of_copy_peak']:.0f} %) | {r['baseline_bytes'] / 1e6:.1f} | "
                    f"{r['baseline_calls']} | {min(r['baseline_us']):.1f}-{max(r['baseline_us']):.1f} | "
                    f"{min(r['fork_eighth_us']):.1f}-{max(r['fork_eighth_us']):.1f} | "
                    f"{'holds' if r['condition_holds'] else 'FAILS'} |")
    return "\n".join([
        "# Fork / restore env state: mc_copy_envs against plain state copies",
        "",
        f"`tools/fork_bench.py`: device events around windows of {res['calls']} calls, {res['reps']} alternating",
        "repetitions in one process; ranges are min-max over the repetitions, in microseconds per call.",
        "Bytes are computed from the shapes (copied state read plus written); GB/s from the median",
        f"repetition, next to the {COPY_PEAK_GBS / 1e3:.2f} TB/s achievable copy rate of one MI355X.  The baseline is",
        "mc_get_state of the maps, positions and per-env scalars into preallocated buffers: what a",
        "whole-batch snapshot costs without the fork (fewer bytes than the fork moves).",
        "",
        "| workload | envs | fork MB | fork us | fork GB/s (of copy peak) | baseline MB | baseline calls | baseline us | "
        "1/8-batch fork us | fork range within baseline range + spread |",
        "|---|---|---|---|---|---|---|---|---|---|",
        *rows,
        "",
        *[f"{name}: the baseline plus plain copies of the registered planes / dist buffers ({r['baseline_buffers_bytes'] / 1e6:.1f} MB, "
          f"the fork's bytes): {min(r['baseline_buffers_us']):.1f}-{max(r['baseline_buffers_us']):.1f} us."
          for name, r in res["workloads"].items() if "baseline_buffers_us" in r],
        "",
        "Raw numbers: `fork_bench.json`.",
        "",
    ])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "fork"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    res = dict(tool="tools/fork_bench.py", calls=a.calls, reps=a.reps, copy_peak_gbs=COPY_PEAK_GBS, workloads={})
    makers = {
        "c2": lambda: dec_workload(torch, 4, 128, 4096, 0),
        "sg_c2": lambda: sg_workload(torch, 128, 4096),
        "c5_256": lambda: dec_workload(torch, 16, 512, 256, 1),
    }
    for name, make in makers.items():
        w = make()
        res["workloads"][name] = measure(torch, w, a.calls, a.reps)
        del w
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "fork_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
