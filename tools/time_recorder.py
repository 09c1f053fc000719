#!/usr/bin/env python3
"""What the device flight recorder (gym_fixed_wing.recorder.FlightRecorder) costs per env step inside a captured rollout: one
replayed FusedRollout graph (two-launch step + HIP head) at 65 536 envs on the `examples` preset (dense observations, MLP head)
and on the `cnn` preset (row log, CNN head), with no recorder, one tracked env and sixteen.  Every figure is one process of its
own (env construction, capture and warm-up replays not timed), reported as the median of 5 such runs.

    python tools/time_recorder.py [--out profiles/recorder_timing.json] [--envs 65536] [--runs 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]
N_STEPS, WARM, REPS = 16, 10, 50


def child(preset, tracked, envs):
    import torch
    from gym_fixed_wing import presets
    from gym_fixed_wing.actor import DeviceActor
    from gym_fixed_wing.recorder import FlightRecorder
    from gym_fixed_wing.rollout import CnnMlpPolicy, FusedRollout, MlpPolicy
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    vec = FixedWingVecEnv(presets.preset(preset), num_envs=envs, device=0, derived_views=preset == "cnn", seed=1)
    if tracked:
        FlightRecorder(vec, env_ids=[i * (envs // tracked) for i in range(tracked)])
    vec.reset()
    actor = DeviceActor.for_env(vec, seed=3)
    torch.manual_seed(0)
    actor.load_policy(CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3).cuda() if preset == "cnn" else MlpPolicy(vec.obs_dim))
    ro = FusedRollout(vec, actor, N_STEPS, graph=True)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.envs)
    out = {"workload": "FusedRollout(graph=True, n_steps={}) at {} envs, two-launch step + HIP head, {} timed replays".format(N_STEPS, args.envs, REPS),
           "method": "one fresh process per figure, median of {}".format(args.runs), "results": []}
    for preset in ("examples", "cnn"):
        row = {"preset": preset}
        for tracked in (0, 1, 16):
            runs = []
            for _ in range(args.runs):   # one process at a time
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--child", preset, str(tracked)],
                                   check=True, capture_output=True, text=True, timeout=300)
                runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            us = [x["us_per_step"] for x in runs]
            row["tracked_{}".format(tracked)] = {"us_per_step_median": statistics.median(us), "us_per_step_min": min(us), "us_per_step_max": max(us)}
        base = row["tracked_0"]["us_per_step_median"]
        row["added_us_per_step"] = {k: row[k]["us_per_step_median"] - base for k in ("tracked_1", "tracked_16")}
        out["results"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
