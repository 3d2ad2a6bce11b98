"""Time SuperGridRL rollouts: K mc_sg_step calls against one mc_sg_step_many
call (csrc/mc_super.hip, sg_step_loop) on the sg_c2 shape without dist_reward
-- 4 robots, 128 x 128, p_obst 0.1, senseradius 2, 4096 envs, auto-reset,
maxsteps 1000 -- with the actions of all K steps staged on the device.

Three paths, on three handles with the same seed (MARLCOV_FUSE_STEPS is read
when a handle is created):
  stepped    K mc_sg_step calls: a step kernel and a distance transform each;
  fused      mc_sg_step_many with the default S (64 steps per launch) and one
             transform per call;
  fused_s1   mc_sg_step_many with S = 1: one step-kernel launch per step,
             still one transform per call.
Before timing, a fused rollout and the stepped twin must end in identical
reward[-1], planes and dist at this size.  Then every path is warmed up, and
device events time windows of K steps, the paths alternating in one process,
--reps repetitions each.  Prints one JSON line and writes it, with a README
(the table, then the directory's notes.md if there is one), into --out.

    python tools/sg_rollout_bench.py [--out DIR] [--steps 256] [--reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SG = dict(numrobot=4, train_maxsteps=1000, test_maxsteps=1000, collision_penalty=5, done_thresh=1, done_incr=0,
          terminal_reward=30, senseradius=2, free_penalty=0.2, dist_reward=0, use_scanning=0)
ENVS, SIDE = 4096, 128


def make_env(fuse):
    import marlcov
    if fuse is None:
        os.environ.pop("MARLCOV_FUSE_STEPS", None)
    else:
        os.environ["MARLCOV_FUSE_STEPS"] = str(fuse)
    env = marlcov.BatchSuperGridEnv(SG, ENVS, gen=dict(width=SIDE, length=SIDE, prob_obst=0.1, seed=1000),
                                    seed=1, auto_reset=True, maxsteps=1000)
    os.environ.pop("MARLCOV_FUSE_STEPS", None)
    env.reset()
    return env


def window_us(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn()
    e1.record()
    torch.cuda.synchronize()
    if rc:
        raise RuntimeError(f"a timed call failed ({rc})")
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "sg_rollout"))
    ap.add_argument("--steps", type=int, default=256, help="K: steps per window")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    K, N = a.steps, SG["numrobot"]
    envs = {"stepped": make_env(None), "fused": make_env(None), "fused_s1": make_env(1)}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    acts = torch.randint(0, 4, (K, ENVS, N), dtype=torch.uint8, device="cuda", generator=g)
    rew = torch.zeros(ENVS, dtype=torch.float64, device="cuda")
    done = torch.zeros(ENVS, dtype=torch.uint8, device="cuda")

    def stepped():
        env, st, rc = envs["stepped"], envs["stepped"]._stream(), 0
        for k in range(K):
            rc |= env.step_raw(acts[k].data_ptr(), rew.data_ptr(), done.data_ptr(), st)
        return rc

    def fused(name):
        env = envs[name]
        return lambda: env.step_many_raw(acts.data_ptr(), ENVS * N, K, rew.data_ptr(), done.data_ptr(), env._stream())

    runs = {"stepped": stepped, "fused": fused("fused"), "fused_s1": fused("fused_s1")}

    # the paths compute the same thing at this size (and serve as a first warm-up)
    last = {}
    for name, fn in runs.items():
        if fn():
            raise RuntimeError(f"{name}: the call failed")
        torch.cuda.synchronize()
        envs[name].check()
        last[name] = rew.clone()
    for name in ("fused", "fused_s1"):
        assert torch.equal(last[name], last["stepped"]), f"{name}: reward[-1] differs from the stepped twin"
        assert torch.equal(envs[name].planes, envs["stepped"].planes), f"{name}: planes differ"
        assert torch.equal(envs[name].dist, envs["stepped"].dist), f"{name}: dist differs"
    launches = {}
    for name, fn in runs.items():  # a second warm-up window, counted
        before = envs[name].launches()
        fn()
        after = envs[name].launches()
        launches[name] = dict(step=after[0] - before[0], dist=after[1] - before[1])
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(a.reps):  # alternate in one process
        for name, fn in runs.items():
            us[name].append(window_us(torch, fn, K))
    for env in envs.values():
        env.check()
    s = us["stepped"]
    spread = max(s) - min(s)
    res = dict(tool="tools/sg_rollout_bench.py", config=dict(SG, envs=ENVS, width=SIDE, length=SIDE, p_obst=0.1,
                                                             auto_reset=True, maxsteps=1000),
               steps_per_window=K, reps=a.reps, kernels=envs["fused"].kernel_variant(),
               launches_per_window=launches, us_per_step=us, identical_results=True,
               speedup_fused_median=sorted(s)[len(s) // 2] / sorted(us["fused"])[len(us["fused"]) // 2],
               # the fused path's max lies below the stepped path's min by more than the stepped path's spread
               condition_holds={n: max(us[n]) < min(s) - spread for n in ("fused", "fused_s1")})
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sg_rollout_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(res, a.out))
    print(json.dumps(res))


def readme(res, out):
    what = {"stepped": "K `mc_sg_step` calls", "fused": "`mc_sg_step_many`, default S = 64",
            "fused_s1": "`mc_sg_step_many`, S = 1"}
    rows = []
    for name, v in res["us_per_step"].items():
        ln = res["launches_per_window"][name]
        cond = "" if name == "stepped" else ("holds" if res["condition_holds"][name] else "FAILS")
        rows.append(f"| {what[name]} | {ln['step']} | {ln['dist']} | {min(v):.2f}-{max(v):.2f} | {cond} |")
    lines = [
        "# SuperGridRL rollouts: mc_sg_step_many against K mc_sg_step calls",
        "",
        f"`tools/sg_rollout_bench.py`: the sg_c2 shape with `dist_reward = 0` ({res['kernels']}), actions staged on",
        f"the device, device events around windows of K = {res['steps_per_window']} steps after a warm-up of every path,",
        f"the paths alternating in one process, {res['reps']} repetitions each; min-max over the repetitions, in",
        "microseconds per step (all 4096 envs).  Before timing, the fused rollouts and the stepped twin ended in",
        "identical `reward[-1]`, `planes` and `dist`.  Condition: the fused path's max lies below the stepped",
        "path's min by more than the stepped path's spread.",
        "",
        "| path | step-kernel launches per window | distance-kernel launches per window | us per step | condition |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"Median speed-up of the default fused path: {res['speedup_fused_median']:.2f}x.  Raw numbers: `sg_rollout_bench.json`.",
        "",
    ]
    notes = os.path.join(out, "notes.md")
    if os.path.exists(notes):
        with open(notes) as f:
            lines += [f.read().rstrip("\n"), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
