"""Time mc_import_maps (csrc/mc_import.hip, ``BatchCoverageEnv.set_global_state``)
against what a user does without it: a torch pack, on the same device, of the
dense planes (nonzero -> bits, the tile and block permutation, the two counts,
the robots' cells; ``torch_pack`` / ``baseline`` below) followed by
``set_state`` of FREE, OBST, VISITED, FREE_COUNT, VISITED_COUNT and POS.

The C2 shape (4 agents, 128 x 128, 4096 envs), layers robots + free + obst (9
planes), two cases: (a) all envs, (b) 64 chosen envs, where the baseline also
pays the ``get_state`` of the whole fields that it cannot avoid (``set_state``
has no per-env form).  The planes are the export of a second handle a few
steps into its episode.  The tool first asserts that both paths leave
identical ``get_state`` fields, then times both: device events around windows
of --calls calls after a warm-up, import and baseline alternating in one
process, --reps repetitions each.  Next to them it records the import's GB/s
(input bytes read plus state bytes written, from the shapes) and the time
mc_export_maps takes for the same layers, which moves the same bytes the other
way (a number, not a gate).  Prints one JSON line and writes it, with a
README, into --out (default profiles/r17/import).

    python tools/import_bench.py [--out DIR] [--calls 20] [--reps 5] [--envs 4096]
    python tools/import_bench.py --rehearse     # no device: the baseline pack against
                                                # marlcov.tiles on the host, the byte counts
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK_GBS = 6290.0  # achievable float4 copy rate of one MI355X (tools/fork_bench.py)

BASE = dict(numrobot=4, maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
            dist_reward=0, train_maxsteps=1000, test_maxsteps=1000, egoradius=2, mini_map_rad=0, comm_radius=0,
            allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=0, sensor_type="lidar",
            sensor_config={"num_lasers": 21, "range": 10})
LAYERS = ("robots", "free", "obst")
CHOSEN = 64


def torch_pack(torch, cells):
    """uint8 cells [..., rows, cols] (nonzero = set) -> int64 tiles [..., TRS, TCS, 4, 4] in the
    device block order: bit 8 r + c of tile (ti, tj) is cell (8 ti + r, 8 tj + c)."""
    rows, cols = cells.shape[-2:]
    trs, tcs = -(-rows // 32), -(-cols // 32)
    lead = tuple(cells.shape[:-2])
    full = torch.nn.functional.pad(cells != 0, (0, 32 * tcs - cols, 0, 32 * trs - rows))
    b = full.reshape(lead + (4 * trs, 8, 4 * tcs, 8)).movedim(-3, -2)  # [..., ti, tj, r, c]
    shifts = torch.arange(64, dtype=torch.int64, device=cells.device).view(8, 8)
    grid = (b.to(torch.int64) << shifts).sum(dim=(-2, -1))  # (distinct bits: the sum wraps to the OR)
    return grid.reshape(lead + (trs, 4, tcs, 4)).movedim(-3, -2).contiguous()


def torch_positions(torch, robots, agents):
    """uint8 robots planes [K, W, L] (i + 1 at robot i's cell) -> int32 [K, agents, 2]"""
    K, W, L = robots.shape
    ids = torch.arange(1, agents + 1, dtype=torch.uint8, device=robots.device).view(1, agents, 1)
    cell = (robots.view(K, 1, W * L) == ids).to(torch.uint8).argmax(dim=-1)
    return torch.stack((cell // L, cell % L), dim=-1).to(torch.int32)


def baseline(torch, env, planes, idx):
    """the import of `planes` (robots, free.., obst..) into the envs `idx` (None: all) without mc_import_maps"""
    from marlcov import _lib
    n = env.num_agents
    free, obst = torch_pack(torch, planes[:, 1:1 + n]), torch_pack(torch, planes[:, 1 + n:])
    union = (planes[:, 1:1 + n] != 0).any(dim=1)
    new = {
        _lib.FIELD_FREE: free, _lib.FIELD_OBST: obst, _lib.FIELD_VISITED: torch_pack(torch, union.to(torch.uint8)),
        _lib.FIELD_FREE_COUNT: (planes[:, 1:1 + n] != 0).sum(dim=(1, 2, 3), dtype=torch.int32),
        _lib.FIELD_VISITED_COUNT: union.sum(dim=(1, 2), dtype=torch.int32),
        _lib.FIELD_POS: torch_positions(torch, planes[:, 0], n),
    }
    for f, t in new.items():
        if idx is not None:  # get, modify, set: the whole field of every env
            whole = env.get_state(f)
            whole[idx] = t
            t = whole
        env.set_state(f, t)


def state_fields(env, idx):
    from marlcov import _lib
    out = []
    for f in (_lib.FIELD_FREE, _lib.FIELD_OBST, _lib.FIELD_VISITED, _lib.FIELD_FREE_COUNT, _lib.FIELD_VISITED_COUNT,
              _lib.FIELD_POS):
        t = env.get_state(f)
        out.append(t if idx is None else t[idx].clone())
    return out


def case_bytes(envs, agents, width, length, map_words):
    """(read, written) bytes of an import of robots + free + obst, from the shapes"""
    read = envs * ((1 + 2 * agents) * width * length + 4 + 4)
    written = envs * ((2 * agents + 1) * map_words * 8 + 8 * agents + 8)
    return read, written


def window_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def measure(torch, env, src, idx, calls, reps, warmup=3):
    """idx: None (all envs) or an int64 device tensor of distinct env indices"""
    planes = src.global_state(LAYERS, envs=idx)
    idx32 = None if idx is None else idx.to(torch.int32)
    out = torch.empty_like(planes)

    def imp():
        env.set_global_state(planes, LAYERS, envs=idx32)

    def base():
        baseline(torch, env, planes, idx)

    def export():
        src.global_state(LAYERS, envs=idx32, out=out)

    # both paths leave identical fields (the env moves on in between, so neither finds the other's result)
    base()
    want = state_fields(env, idx)
    env.step(env.random_actions(99, 0))
    imp()
    got = state_fields(env, idx)
    env.check()
    if not all(torch.equal(a, b) for a, b in zip(got, want)):
        raise RuntimeError("import and torch baseline leave different fields")
    if not torch.equal(env.global_state(LAYERS, envs=idx32)[:, 1:] != 0, planes[:, 1:] != 0):
        raise RuntimeError("the imported state does not export to the planes")
    for fn in (imp, base, export):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {"import": [], "baseline": [], "export": []}
    for _ in range(reps):  # alternate in one process
        us["import"].append(window_us(torch, imp, calls))
        us["baseline"].append(window_us(torch, base, max(1, calls // 4)))
        us["export"].append(window_us(torch, export, calls))
    env.check()
    K = planes.shape[0]
    read, written = case_bytes(K, env.num_agents, env.width, env.length, int(env.layout.mask_words_per_agent))
    med = sorted(us["import"])[reps // 2]
    return dict(layers=list(LAYERS), envs=K, of_envs=env.num_envs, planes=int(planes.shape[1]), read_bytes=read,
                written_bytes=written, import_us=us["import"], baseline_us=us["baseline"], export_us=us["export"],
                import_gbs=(read + written) / med / 1e3,
                import_share_of_copy_peak=(read + written) / med / 1e3 / COPY_PEAK_GBS,
                speedup_median=sorted(us["baseline"])[reps // 2] / med,
                # the import's slowest repetition is not slower than the baseline's fastest
                condition_holds=max(us["import"]) <= min(us["baseline"]))


def readme(res):
    rows = []
    for name, r in res["cases"].items():
        rows.append(f"| {name} | {r['envs']} of {r['of_envs']} | {r['read_bytes'] / 1e6:.1f} | "
                    f"{r['written_bytes'] / 1e6:.1f} | {min(r['import_us']):.1f}-{max(r['import_us']):.1f} | "
                    f"{r['import_gbs']:.0f} ({100 * r['import_share_of_copy_peak']:.0f} %) | "
                    f"{min(r['export_us']):.1f}-{max(r['export_us']):.1f} | "
                    f"{min(r['baseline_us']):.0f}-{max(r['baseline_us']):.0f} | {r['speedup_median']:.0f}x | "
                    f"{'holds' if r['condition_holds'] else 'FAILS'} |")
    return "\n".join([
        "# Dense planes into the env state: mc_import_maps against a torch pack and set_state",
        "",
        f"`tools/import_bench.py`, C2 shape ({res['envs']} envs, 4 agents, 128 x 128), layers robots + free + obst (9",
        f"planes): device events around windows of {res['calls']} calls (baseline: a quarter as many), {res['reps']} alternating",
        "repetitions in one process; ranges are min-max over the repetitions, in microseconds per call.  The",
        "baseline is a torch pack on the same device (nonzero -> bits, the tile and block permutation, the two",
        "counts, the robots' cells) followed by `set_state` of FREE, OBST, VISITED, FREE_COUNT, VISITED_COUNT and",
        "POS; for the chosen envs it includes the `get_state` of the whole fields, which it cannot avoid.  The tool",
        "asserts that both paths leave identical `get_state` fields before it times either.  Bytes are computed",
        "from the shapes (planes read; tile words, positions and counters written); GB/s from the median",
        f"repetition, next to the {COPY_PEAK_GBS / 1e3:.2f} TB/s achievable copy rate of one MI355X.  `export us` is",
        "`mc_export_maps` of the same layers and envs, which moves the same bytes the other way (numbers, not gates).",
        "",
        "Condition: the import's slowest repetition is not slower than the baseline's fastest.",
        "",
        "| case | envs | read MB | written MB | import us | import GB/s (of copy peak) | export us | baseline us | median speed-up | condition |",
        "|---|---|---|---|---|---|---|---|---|---|",
        *rows,
        "",
        ("The condition holds for every case." if all(r["condition_holds"] for r in res["cases"].values())
         else "The condition FAILS for: " + ", ".join(n for n, r in res["cases"].items() if not r["condition_holds"])),
        "",
        "Raw numbers: `import_bench.json`.",
        "",
    ])


def rehearse():
    """No device: the baseline's pack against marlcov.tiles on the host, and the byte counts."""
    import numpy as np
    import torch
    from marlcov.tiles import cells_to_tiles
    rs = np.random.RandomState(0)
    cells = rs.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=(3, 2, 130, 130))
    got = torch_pack(torch, torch.from_numpy(cells)).numpy()
    want = cells_to_tiles(cells, blocks=True).view(np.int64)
    assert got.shape == want.shape == (3, 2, 5, 5, 4, 4) and np.array_equal(got, want), "torch_pack differs from cells_to_tiles"
    robots = np.zeros((2, 130, 130), dtype=np.uint8)
    pos = np.array([[[1, 1], [128, 128], [64, 3], [5, 77]], [[9, 9], [9, 10], [100, 1], [1, 100]]])
    for k in range(2):
        for i in range(4):
            robots[k, pos[k, i, 0], pos[k, i, 1]] = i + 1
    assert np.array_equal(torch_positions(torch, torch.from_numpy(robots), 4).numpy(), pos)
    print("all envs read, written bytes:", case_bytes(4096, 4, 130, 130, 400))
    print("chosen envs read, written bytes:", case_bytes(CHOSEN, 4, 130, 130, 400))
    print("rehearsal ok (no timing without a device)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "import"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    import torch
    import marlcov
    if not torch.cuda.is_available():
        raise SystemExit("import_bench: no HIP device (timings need one; --rehearse runs the host checks)")
    gen = dict(width=128, length=128, prob_obst=0.1, seed=1000)
    src = marlcov.BatchCoverageEnv(BASE, a.envs, gen=gen, seed=1, auto_reset=True)
    env = marlcov.BatchCoverageEnv(BASE, a.envs, gen=gen, seed=2, auto_reset=True)
    src.reset()
    env.reset()
    for t in range(6):
        src.step(src.random_actions(7, t))
    env.step(env.random_actions(8, 0))
    chosen = torch.arange(CHOSEN, dtype=torch.int64, device=env.device) * (a.envs // CHOSEN) + 3 % max(1, a.envs // CHOSEN)
    res = dict(tool="tools/import_bench.py", calls=a.calls, reps=a.reps, envs=a.envs, copy_peak_gbs=COPY_PEAK_GBS,
               cases={})
    for name, idx in (("all_envs", None), (f"chosen_{CHOSEN}", chosen)):
        res["cases"][name] = measure(torch, env, src, idx, a.calls, a.reps)
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "import_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
