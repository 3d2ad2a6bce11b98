"""Step time of dijkstra_input on the reference's 1073x1073 map, where the
full-map BFS keeps its planes in HBM (csrc/mc_dijkstra.hip
dijkstra_big_kernel): mc_step_many between HIP events, one process.

    python tools/dj_big_probe.py [--envs 64] [--agents 4] [--steps 20] [--warmup 3] [--depth 120]

Two cases, one JSON line each:
  empty   right after a reset: every path is inside the window kernel's 24
          layers, the list is empty and the HBM kernel runs over zero items;
  listed  maps explored within L1 distance --depth of each robot injected
          first: every (env, agent) is listed and solved on the whole map.
"hbm_share" of the listed case is the part of its step above the empty
case's step (the window kernel and the env kernel run in both).  The process
ends itself (SIGALRM) after --timeout seconds.
"""
import argparse
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(numrobot=4, maxsteps=100000, collision_penalty=5, done_thresh=1, done_incr=0, terminal_reward=30,
           dist_reward=0, train_maxsteps=100000, test_maxsteps=100000, egoradius=2, mini_map_rad=0, comm_radius=0,
           allow_comm=0, map_sharing=0, single_square_tool=0, dijkstra_input=1, sensor_type="lidar",
           sensor_config={"num_lasers": 21, "range": 10})


def inject(torch, env, neg, depth):
    """Maps explored within L1 distance `depth` of each robot, env by env."""
    from marlcov import _lib
    from marlcov.tiles import cells_to_tiles
    B, N, W, L = env.num_envs, env.num_agents, env.width, env.length
    pos = env.get_state(_lib.FIELD_POS).cpu().numpy()
    X, Y = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(L, dtype=np.int32), indexing="ij")
    shape = env.field_shape(_lib.FIELD_FREE)
    ft, ot = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
    vt = np.zeros(env.field_shape(_lib.FIELD_VISITED), np.uint64)
    fc, vc = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        near = np.stack([(np.abs(X - x) + np.abs(Y - y)) < depth for x, y in pos[b]])
        free, obst = near & (neg == 0), near & (neg == 1)
        ft[b], ot[b] = cells_to_tiles(free, blocks=True), cells_to_tiles(obst, blocks=True)
        vt[b] = cells_to_tiles(free.max(axis=0), blocks=True)
        fc[b], vc[b] = free.sum(), free.max(axis=0).sum()
    for f, a in ((_lib.FIELD_FREE, ft.view(np.int64)), (_lib.FIELD_OBST, ot.view(np.int64)),
                 (_lib.FIELD_VISITED, vt.view(np.int64)), (_lib.FIELD_FREE_COUNT, fc),
                 (_lib.FIELD_VISITED_COUNT, vc)):
        env.set_state(f, torch.from_numpy(a))


def timed(torch, env, K, W, seed):
    from marlcov import _lib
    B, N = env.num_envs, env.num_agents
    acts = torch.empty((W + K, B, N), dtype=torch.uint8, device=env.device)
    for i in range(W + K):
        env.random_actions(seed, i, out=acts[i])
    sp = torch.cuda.current_stream(env.device).cuda_stream
    rp, dp, op = env.reward.data_ptr(), env.done.data_ptr(), env.obs.data_ptr()
    assert env.step_many_raw(acts[0].data_ptr(), B * N, W, rp, dp, op, sp) == 0
    torch.cuda.synchronize(env.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert env.step_many_raw(acts[W].data_ptr(), B * N, K, rp, dp, op, sp) == 0
    e1.record()
    torch.cuda.synchronize(env.device)
    env.check()
    return e0.elapsed_time(e1) / K * 1e3, int(env.get_state(_lib.FIELD_DJ_LISTED).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=120)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.timeout)

    import torch

    import marlcov
    _, test = marlcov.gridload({"grid_dir": os.path.join(ROOT, "tests", "golden", "maps"), "numgrids": 1000},
                               sort=True)
    g = [m for m in test if m.shape == (1073, 1073)][0]
    cfg = dict(CFG, numrobot=args.agents)
    env = marlcov.BatchCoverageEnv(cfg, args.envs, grids=[g], auto_reset=False, seed=1)
    base = {"map": "bg2_1073x1073", "envs": args.envs, "agents": args.agents, "steps": args.steps,
            "warmup": args.warmup, "dijkstra_variant": env.dijkstra_variant()}
    env.reset()
    us0, listed0 = timed(torch, env, args.steps, args.warmup, 5)
    print(json.dumps(dict(base, case="empty", us_per_step=round(us0, 2), listed_last_step=listed0)), flush=True)
    env.reset()
    neg = np.pad(np.asarray(g), 1, constant_values=-1) < 0
    inject(torch, env, neg, args.depth)
    us1, listed1 = timed(torch, env, args.steps, args.warmup, 5)
    print(json.dumps(dict(base, case="listed", depth=args.depth, us_per_step=round(us1, 2),
                          listed_last_step=listed1, hbm_share=round(max(0.0, 1 - us0 / us1), 4))), flush=True)


if __name__ == "__main__":
    main()
