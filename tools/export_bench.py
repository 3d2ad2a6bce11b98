"""Time mc_export_maps (csrc/mc_export.hip, ``BatchCoverageEnv.global_state``)
against what a user does without it: a torch decode, on the same device, of
the ``get_state`` tensors -- shifts and masks of the int64 tiles, the
block-to-tile permutation, the crop (``torch_decode`` below).

The C2 shape (4 agents, 128 x 128, 4096 envs, a few random steps first), three
cases: (a) the default three layers at scale 1, (b) MC_MAP_ALL at scale 1, (c)
the default layers at scale 8.  The tool first asserts that the baseline equals
the export bit for bit, then times both: device events around windows of
--calls calls after a warm-up, export and baseline alternating in one process,
--reps repetitions each.  Bytes are computed from the shapes: the tile words
(and positions) the layers read plus the output bytes written.  Prints one JSON
line and writes it, with a README, into --out (default profiles/r16/export).

    python tools/export_bench.py [--out DIR] [--calls 20] [--reps 5] [--envs 4096]
    python tools/export_bench.py --rehearse     # no device: the baseline decode against
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
DEFAULT = ("visited", "obst_any", "robots")
ORDER = ("grid_neg", "grid_pos", "visited", "obst_any", "robots", "free", "obst")


def torch_decode(torch, tiles, rows, cols):
    """int64 tiles [..., TRS, TCS, 4, 4] (device block order) -> uint8 cells
    [..., rows, cols]: bit 8 r + c of tile (ti, tj) is cell (8 ti + r, 8 tj + c)."""
    lead, (trs, tcs) = tuple(tiles.shape[:-4]), tuple(tiles.shape[-4:-2])
    grid = tiles.movedim(-2, -3).reshape(lead + (4 * trs, 4 * tcs))
    shifts = torch.arange(64, dtype=torch.int64, device=tiles.device).view(8, 8)
    bits = ((grid[..., None, None] >> shifts) & 1).to(torch.uint8)  # [..., ti, tj, r, c]
    return bits.movedim(-2, -3).reshape(lead + (32 * trs, 32 * tcs))[..., :rows, :cols]


def torch_pool8(torch, dense):
    """uint8 [..., W, L] -> uint8 [..., ceil(W / 8), ceil(L / 8)] block sums, zero-padded"""
    W, L = dense.shape[-2:]
    tr, tc = -(-W // 8), -(-L // 8)
    full = torch.nn.functional.pad(dense, (0, 8 * tc - L, 0, 8 * tr - W))
    return full.reshape(tuple(dense.shape[:-2]) + (tr, 8, tc, 8)).sum(dim=(-3, -1), dtype=torch.int32).to(torch.uint8)


def baseline_planes(torch, env, layers, out):
    """`out` uint8 [B, P, W, L]: the planes of `layers` decoded with torch from get_state"""
    from marlcov import _lib
    W, L, N = env.width, env.length, env.num_agents
    p = 0
    obst = env.get_state(_lib.FIELD_OBST) if ("obst_any" in layers or "obst" in layers) else None
    for name in ORDER:
        if name not in layers:
            continue
        if name in ("grid_neg", "grid_pos"):
            f = _lib.FIELD_GRID_NEG if name == "grid_neg" else _lib.FIELD_GRID_POS
            eg = env.get_state(_lib.FIELD_ENV_GRID).long()
            out[:, p] = torch_decode(torch, env.get_state(f)[eg], W, L)
        elif name == "visited":
            out[:, p] = torch_decode(torch, env.get_state(_lib.FIELD_VISITED), W, L)
        elif name == "obst_any":
            anyo = obst[:, 0]
            for i in range(1, N):
                anyo = anyo | obst[:, i]
            out[:, p] = torch_decode(torch, anyo, W, L)
        elif name == "robots":
            pos = env.get_state(_lib.FIELD_POS).long()
            plane = torch.zeros((env.num_envs, W * L), dtype=torch.uint8, device=out.device)
            ids = torch.arange(1, N + 1, dtype=torch.uint8, device=out.device).expand(env.num_envs, N)
            plane.scatter_(1, pos[..., 0] * L + pos[..., 1], ids)
            out[:, p] = plane.view(-1, W, L)
        elif name == "free":
            out[:, p:p + N] = torch_decode(torch, env.get_state(_lib.FIELD_FREE), W, L)
            p += N - 1
        else:
            out[:, p:p + N] = torch_decode(torch, obst, W, L)
            p += N - 1
        p += 1
    return out


def case_bytes(layers, scale, envs, agents, width, length, map_words):
    """(read, written) bytes of an export, from the shapes"""
    words = sum({"grid_neg": 1, "grid_pos": 1, "visited": 1, "obst_any": agents, "robots": 0, "free": agents,
                 "obst": agents}[n] for n in layers)
    planes = sum(agents if n in ("free", "obst") else 1 for n in layers)
    plane = width * length if scale == 1 else -(-width // 8) * -(-length // 8)
    read = envs * (words * map_words * 8 + (8 * agents if "robots" in layers else 0) + 4)
    return read, envs * planes * plane


def window_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def measure(torch, env, layers, scale, calls, reps, warmup=3):
    B, W, L = env.num_envs, env.width, env.length
    P = len(env.global_state_planes(layers))
    out = env.global_state(layers, scale=scale)
    dense = torch.empty((B, P, W, L), dtype=torch.uint8, device=env.device)
    robots = env.global_state_planes(layers).index("robots")

    def export():
        env.global_state(layers, scale=scale, out=out)

    def baseline():
        baseline_planes(torch, env, layers, dense)
        if scale == 1:
            return dense
        d = dense.clone()
        d[:, robots] = d[:, robots] != 0
        return torch_pool8(torch, d)

    export()
    want = baseline()
    if not torch.equal(out, want):
        raise RuntimeError(f"export and torch baseline differ ({layers}, scale {scale})")
    for fn in (export, baseline):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {"export": [], "baseline": []}
    for _ in range(reps):  # alternate in one process
        us["export"].append(window_us(torch, export, calls))
        us["baseline"].append(window_us(torch, baseline, max(1, calls // 4)))
    env.check()
    read, written = case_bytes(layers, scale, B, env.num_agents, W, L, int(env.layout.mask_words_per_agent))
    med = sorted(us["export"])[reps // 2]
    return dict(layers=list(layers), scale=scale, envs=B, planes=P, read_bytes=read, written_bytes=written,
                export_us=us["export"], baseline_us=us["baseline"], export_gbs=(read + written) / med / 1e3,
                export_share_of_copy_peak=(read + written) / med / 1e3 / COPY_PEAK_GBS,
                speedup_median=sorted(us["baseline"])[reps // 2] / med,
                # the export's slowest repetition is not slower than the baseline's fastest
                condition_holds=max(us["export"]) <= min(us["baseline"]))


def readme(res):
    rows = []
    for name, r in res["cases"].items():
        rows.append(f"| {name} | {r['planes']} | {r['read_bytes'] / 1e6:.1f} | {r['written_bytes'] / 1e6:.1f} | "
                    f"{min(r['export_us']):.1f}-{max(r['export_us']):.1f} | {r['export_gbs']:.0f} "
                    f"({100 * r['export_share_of_copy_peak']:.0f} %) | {min(r['baseline_us']):.0f}-{max(r['baseline_us']):.0f} | "
                    f"{r['speedup_median']:.0f}x | {'holds' if r['condition_holds'] else 'FAILS'} |")
    return "\n".join([
        "# Global state on the device: mc_export_maps against a torch decode of get_state",
        "",
        f"`tools/export_bench.py`, C2 shape ({res['envs']} envs, 4 agents, 128 x 128): device events around windows of",
        f"{res['calls']} calls (baseline: a quarter as many), {res['reps']} alternating repetitions in one process; ranges are",
        "min-max over the repetitions, in microseconds per call.  The baseline is a torch decode on the same",
        "device of the `get_state` tensors (shifts and masks of the int64 tiles, the block-to-tile permutation,",
        "the crop); the tool asserts that it equals the export bit for bit before it times either.  Bytes are",
        "computed from the shapes (tile words and positions read plus output written); GB/s from the median",
        f"repetition, next to the {COPY_PEAK_GBS / 1e3:.2f} TB/s achievable copy rate of one MI355X (a number, not a gate).",
        "",
        "Condition: the export's slowest repetition is not slower than the baseline's fastest.",
        "",
        "| case | planes | read MB | written MB | export us | export GB/s (of copy peak) | baseline us | median speed-up | condition |",
        "|---|---|---|---|---|---|---|---|---|",
        *rows,
        "",
        ("The condition holds for every case." if all(r["condition_holds"] for r in res["cases"].values())
         else "The condition FAILS for: " + ", ".join(n for n, r in res["cases"].items() if not r["condition_holds"])),
        "",
        "Raw numbers: `export_bench.json`.",
        "",
    ])


def rehearse():
    """No device: the baseline's decode against marlcov.tiles on the host, and the byte counts."""
    import numpy as np
    import torch
    from marlcov.tiles import tiles_to_cells
    rs = np.random.RandomState(0)
    tiles = rs.randint(-2 ** 63, 2 ** 63 - 1, size=(3, 2, 5, 5, 4, 4), dtype=np.int64)
    got = torch_decode(torch, torch.from_numpy(tiles), 130, 130).numpy()
    assert np.array_equal(got, tiles_to_cells(tiles, 130, 130)), "torch_decode differs from tiles_to_cells"
    pooled = torch_pool8(torch, torch.from_numpy(got)).numpy()
    full = np.zeros((3, 2, 136, 136), dtype=np.int64)
    full[..., :130, :130] = got
    assert np.array_equal(pooled, full.reshape(3, 2, 17, 8, 17, 8).sum(axis=(3, 5)))
    for name, layers, scale in CASES:
        print(name, "read, written bytes:", case_bytes(layers, scale, 4096, 4, 130, 130, 400))
    print("rehearsal ok (no timing without a device)")


CASES = [("default_dense", DEFAULT, 1), ("all_dense", ORDER, 1), ("default_pooled", DEFAULT, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "export"))
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
        raise SystemExit("export_bench: no HIP device (timings need one; --rehearse runs the host checks)")
    env = marlcov.BatchCoverageEnv(BASE, a.envs, gen=dict(width=128, length=128, prob_obst=0.1, seed=1000), seed=1,
                                   auto_reset=True)
    env.reset()
    for t in range(6):
        env.step(env.random_actions(7, t))
    res = dict(tool="tools/export_bench.py", calls=a.calls, reps=a.reps, envs=a.envs, copy_peak_gbs=COPY_PEAK_GBS,
               cases={})
    for name, layers, scale in CASES:
        res["cases"][name] = measure(torch, env, layers, scale, a.calls, a.reps)
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "export_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
