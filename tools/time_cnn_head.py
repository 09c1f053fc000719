#!/usr/bin/env python3
"""The CNN head against the MLP head on the benchmark's env (c3_cnn_step2_dryden_log: 65 536 envs, cnn preset, observation step 2,
Dryden moderate, 5 x 12 row log read in place), in the same process:

  act       one fwg_actor_act (k_actor_act_cnn<3> vs k_actor_act<3, 4> on the flattened window), HIP events, median of 200
  rollout   one rollout step of a captured FusedRollout (env step + batch moments + head), 64-step graph replays

    python tools/time_cnn_head.py [--envs 65536] [--out FILE.json]     (one JSON line on stdout; profiles/cnn_head_timing.json)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_fixed_wing import presets  # noqa: E402
from gym_fixed_wing.actor import DeviceActor  # noqa: E402
from gym_fixed_wing.rollout import CnnMlpPolicy, FusedRollout, MlpPolicy  # noqa: E402
from gym_fixed_wing.vec_env import FixedWingVecEnv  # noqa: E402


def make_vec(n):
    cfg, ckw, skw, _, _ = presets.workload("c3")
    return FixedWingVecEnv(cfg, num_envs=n, device=0, config_kw=ckw, sim_config_kw=skw, seed=1, derived_views=False,
                           obs_log_rows=presets.OBS_LOG_ROWS)


def time_act(vec, pol, reps=200):
    a = DeviceActor.for_env(vec, seed=1, training=False)
    a.load_policy(pol)
    a.set_obs_log(vec)
    n = vec.num_envs
    outs = [torch.zeros((n, 60), device="cuda"), torch.zeros((n, 3), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    for _ in range(10):
        a.act(vec._obs_buf, norm_obs=outs[0], action=outs[1], value=outs[2], logp=outs[3])
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        a.act(vec._obs_buf, norm_obs=outs[0], action=outs[1], value=outs[2], logp=outs[3])
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    a.close()
    return float(np.median(ts))


def time_rollout(vec, pol, steps=64, reps=6):
    a = DeviceActor.for_env(vec, seed=1)
    a.load_policy(pol)
    ro = FusedRollout(vec, a, steps, graph=True)
    ro.run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ro.run()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / steps)
    a.close()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--out", default=None, help="also write the result here")
    args = ap.parse_args()
    torch.manual_seed(0)
    pols = {"mlp": MlpPolicy(60).cuda(), "cnn": CnnMlpPolicy().cuda()}
    vec = make_vec(args.envs)
    vec.reset()
    for _ in range(8):
        vec.step_device(torch.zeros((args.envs, 3), device="cuda"))
    out = {"envs": args.envs, "workload": "c3_cnn_step2_dryden_log"}
    for name, pol in pols.items():   # interleaved twice: drift shows up as a difference between the two rounds
        out.setdefault("act_us_" + name, []).append(time_act(vec, pol))
    for name, pol in pols.items():
        out.setdefault("rollout_step_us_" + name, []).append(time_rollout(vec, pol))
    for name, pol in pols.items():
        out["act_us_" + name].append(time_act(vec, pol))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    vec.close()


if __name__ == "__main__":
    main()
