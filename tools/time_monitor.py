#!/usr/bin/env python3
"""What the device training monitor (gym_fixed_wing.monitor) costs, at 65 536 envs x 128 steps:

  1. one captured rollout step (FusedRollout(graph=True), two-launch step + HIP head) with and without raw_rewards, on the
     `examples` preset (dense observations, MLP head) and on the `cnn` preset (row log, CNN head) -- the flag sends the same bytes
     to another address, so no difference beyond the run-to-run spread is expected;
  2. fwg_monitor_fold beside fwg_gae on the same shape in the same process (5 B per transition against 17).

Every figure is one process of its own (construction, capture and warm-up not timed), reported as the median of 5 such runs.

    python tools/time_monitor.py [--out profiles/monitor_timing.json] [--envs 65536] [--runs 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]
N_STEPS, WARM, REPS = 128, 3, 20
FOLD_WARM, FOLD_REPS = 20, 200


def child_rollout(preset, raw, envs):
    import torch
    from gym_fixed_wing import presets
    from gym_fixed_wing.actor import DeviceActor
    from gym_fixed_wing.rollout import CnnMlpPolicy, FusedRollout, MlpPolicy
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    vec = FixedWingVecEnv(presets.preset(preset), num_envs=envs, device=0, derived_views=preset == "cnn", seed=1)
    vec.reset()
    actor = DeviceActor.for_env(vec, seed=3)
    torch.manual_seed(0)
    actor.load_policy(CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3).cuda() if preset == "cnn" else MlpPolicy(vec.obs_dim))
    ro = FusedRollout(vec, actor, N_STEPS, graph=True, raw_rewards=bool(raw))
    for _ in range(WARM):
        ro.run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPS):
        ro.run()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"us_per_step": 1e3 * t0.elapsed_time(t1) / (REPS * N_STEPS), "fused": bool(ro.fused), "spec": vec.spec_index}))


def child_fold(envs):
    """fwg_monitor_fold and fwg_gae on one [128][envs] rollout, alternating blocks of launches under device events."""
    import types
    import torch
    from gym_fixed_wing import _native as nat
    from gym_fixed_wing.monitor import EpisodeMonitor
    from gym_fixed_wing.ppo import gae
    from gym_fixed_wing.vec_env import _TorchBackend
    lib, mem = nat.load_library(), _TorchBackend(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    rew = torch.randn((N_STEPS, envs), device="cuda", generator=g)
    val = torch.randn((N_STEPS, envs), device="cuda", generator=g)
    done = (torch.rand((N_STEPS, envs), device="cuda", generator=g) < 0.01).to(torch.uint8)
    last = torch.randn((envs,), device="cuda", generator=g)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    m = EpisodeMonitor(types.SimpleNamespace(_lib=lib, _mem=mem, num_envs=envs, _monitor=None))
    runs = {"fwg_monitor_fold": lambda: m.fold(rew, done), "fwg_gae": lambda: gae(lib, mem, rew, val, done, last, 0.99, 0.95, adv, ret)}
    us = {k: [] for k in runs}
    for name, call in runs.items():
        for _ in range(FOLD_WARM):
            call()
    torch.cuda.synchronize()
    for block in range(4):                       # alternating: fold, gae, fold, gae ...
        for name, call in runs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(FOLD_REPS):
                call()
            t1.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * t0.elapsed_time(t1) / FOLD_REPS)
    took = m.take()
    print(json.dumps({"us": {k: statistics.median(v) for k, v in us.items()}, "episodes_folded": took["episodes"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_fold(args.envs) if args.child[0] == "fold" else child_rollout(args.child[0], int(args.child[1]), args.envs)

    def fresh(*what):   # one process at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--child"] + [str(w) for w in what],
                           check=True, capture_output=True, text=True, timeout=300)
        return json.loads(r.stdout.strip().splitlines()[-1])

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    out = {"shape": "{} envs x {} steps".format(args.envs, N_STEPS), "method": "one fresh process per figure, median of {}".format(args.runs),
           "rollout": {"workload": "FusedRollout(graph=True, n_steps={}), two-launch step + HIP head, {} timed replays".format(N_STEPS, REPS),
                       "results": []}}
    folds = [fresh("fold") for _ in range(args.runs)]
    out["fold"] = {"workload": "{} launches per block, 4 alternating blocks per process, device events".format(FOLD_REPS),
                   "bytes_per_transition": {"fwg_monitor_fold": 5, "fwg_gae": 17},
                   "us": {k: spread([f["us"][k] for f in folds]) for k in ("fwg_monitor_fold", "fwg_gae")}}
    print(json.dumps(out["fold"]), flush=True)
    for preset in ("examples", "cnn"):
        runs = {0: [], 1: []}
        for _ in range(args.runs):
            for raw in (0, 1):                   # alternating: the two figures of a pair share the machine's state
                runs[raw].append(fresh(preset, raw)["us_per_step"])
        row = {"preset": preset, "us_per_step": {"plain": spread(runs[0]), "raw_rewards": spread(runs[1])}}
        row["difference_us"] = row["us_per_step"]["raw_rewards"]["median"] - row["us_per_step"]["plain"]["median"]
        out["rollout"]["results"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
