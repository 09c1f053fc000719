#!/usr/bin/env python3
"""Times one PPO update of each path -- torch autograd (PPO(update="torch"), the default, each minibatch step a replayed graph)
and the HIP kernels (PPO(update="hip"), the whole update one replayed graph) -- in the same process on the same GPU, on bench.py's
`c5_train` recipe: workload c5 (65 536 envs), n_steps 128, 4 epochs x 128 minibatches, lr 5e-4.  Both learners train on the
same collected batch; each path is warmed up (graph capture) by one update, then timed over `--updates` updates (median).
--policy cnn: the CNN controller instead -- CnnMlpPolicy (examples/train_ppo.py's) on the cnn configuration at 65 536 envs, the
same recipe, update="torch" against update="hip_cnn"; --policy mlp60: the MlpPolicy on that configuration's flattened 60
observations (what the CNN learner's extra work is measured against).  Prints one JSON line.

    timeout -k 10 600 python tools/time_ppo_update.py [--policy mlp|cnn|mlp60] [--updates 5] [--out result.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_ppo_update.py --paths hip --updates 1"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

import torch  # noqa: E402

from gym_fixed_wing import presets  # noqa: E402
from gym_fixed_wing.ppo import PPO, sb_init_  # noqa: E402
from gym_fixed_wing.rollout import CnnMlpPolicy  # noqa: E402
from gym_fixed_wing.vec_env import FixedWingVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--paths", default="torch,hip")
    ap.add_argument("--out", default=None)
    ap.add_argument("--policy", choices=("mlp", "cnn", "mlp60"), default="mlp")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.policy == "mlp":
        cfg, ckw, skw, n, desc = presets.workload("c5")
        vec = FixedWingVecEnv(cfg, num_envs=n, config_kw=ckw, sim_config_kw=skw, seed=0, device=0)
    else:   # (examples/train_ppo.py --policy cnn: the shipped cnn configuration, derived views on)
        n = 65536
        vec = FixedWingVecEnv(presets.preset("cnn"), num_envs=n, derived_views=True, seed=0, device=0)
    vec.reset()
    res = {"workload": "c5" if args.policy == "mlp" else "cnn", "policy": args.policy, "envs": n, "n_steps": 128, "nminibatches": 128, "noptepochs": 4, "learning_rate": 5e-4,
           "transitions_per_update": 128 * n, "updates_timed": args.updates}
    batch = None
    for path in args.paths.split(","):
        net = None
        if args.policy == "cnn":
            torch.manual_seed(0)
            net = sb_init_(CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3))
        ppo = PPO(vec, policy=net, seed=0, nminibatches=128, learning_rate=5e-4,
                  update="hip_cnn" if (path == "hip" and net is not None) else path)
        if batch is None:   # one rollout, shared by both paths (copied: each update reads it, neither writes it)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            batch = {k: v.clone() for k, v in ppo.collect().items()}
            torch.cuda.synchronize(dev)
            res["rollout_ms"] = (time.perf_counter() - t0) * 1e3
            ppo.collect()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            ppo.collect()
            torch.cuda.synchronize(dev)
            res["rollout_ms"] = (time.perf_counter() - t0) * 1e3   # (the second, captured one)
        b = {k: v.clone() for k, v in batch.items()}
        ppo.update(b)            # warm-up: graph capture
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(args.updates):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            stats = ppo.update(b)
            e1.record()
            torch.cuda.synchronize(dev)
            ts.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        ts.sort()
        wall, gpu = ts[len(ts) // 2]
        res[path] = {"update_ms": wall, "update_ms_events": gpu, "all_ms": [round(t[0], 3) for t in ts],
                     "ms_per_minibatch_step": wall / (4 * 128), "stats": stats}
        del ppo
    if "torch" in res and "hip" in res:
        res["speedup"] = res["torch"]["update_ms"] / res["hip"]["update_ms"]
        per = res["hip"]["update_ms"] + res.get("rollout_ms", 0.0)
        res["hip_train_ms_per_update_incl_rollout"] = per
        res["hip_train_env_steps_per_s"] = 128 * n / (per * 1e-3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    vec.close()


if __name__ == "__main__":
    main()
