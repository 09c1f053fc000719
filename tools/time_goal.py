#!/usr/bin/env python3
"""What the goal env (gym_fixed_wing.goal) costs, at 65 536 envs x 128 steps on the `default` preset with the goals roll / pitch / Va:

  1. one captured rollout step (FusedRollout(graph=True, raw_rewards=True), two-launch step + HIP head) with and without a GoalLog,
     both in the same process, alternating blocks of replays: the log adds one fwg_goal_observe launch per step;
  2. fwg_goal_relabel (p = 0.8) beside fwg_gae on the same rollout's buffers, as us and as the bandwidth its own algorithmic byte
     count comes to (53 B per transition for the scan launch, 12 B per transition and 60 B more per relabelled
     one for the reward launch; the 8x line amplification of the 16-B gather is NOT in that count);
  3. fwg_goal_reward at m = envs x 128 transitions (the batched compute_reward of a replay buffer).

Every run is one process of its own (construction, capture and warm-up not timed); the figures are the medians of 5 such runs.

    python tools/time_goal.py [--out profiles/goal_timing.json] [--envs 65536] [--runs 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]
N_STEPS, WARM, REPS, BLOCKS = 128, 3, 10, 3
K_WARM, K_REPS = 10, 50
GOALS = [{"name": "roll", "mean": 0.0, "var": 1.0}, {"name": "pitch", "mean": 0.0, "var": 0.5}, {"name": "Va", "mean": 22.0, "var": 10.0}]
BYTES = {"scan": 53, "reward_any": 12, "reward_relabelled": 60, "fwg_gae": 17, "fwg_goal_reward": 16 + 16 + 4 + 4}   # (+ 16 W: the window)


def timed(call, reps):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps


def child(envs):
    import ctypes
    import torch
    from gym_fixed_wing import _native as nat
    from gym_fixed_wing import presets
    from gym_fixed_wing.actor import DeviceActor
    from gym_fixed_wing.goal import GoalLog, goal_window
    from gym_fixed_wing.ppo import gae
    from gym_fixed_wing.rollout import FusedRollout, MlpPolicy
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    cfg = presets.preset("default")
    cfg["observation"]["goals"] = GOALS
    runs = {}
    for name in ("plain", "goal_log"):
        vec = FixedWingVecEnv(cfg, num_envs=envs, device=0, seed=1)
        vec.reset()
        actor = DeviceActor.for_env(vec, seed=3)
        torch.manual_seed(0)
        actor.load_policy(MlpPolicy(vec.obs_dim))
        log = GoalLog(vec, N_STEPS) if name == "goal_log" else None
        ro = FusedRollout(vec, actor, N_STEPS, graph=True, raw_rewards=True, goals=log)
        for _ in range(WARM):
            ro.run()
        runs[name] = (vec, ro, log)
    torch.cuda.synchronize()
    us = {name: [] for name in runs}
    for _ in range(BLOCKS):                      # alternating: plain, goal_log, plain ...
        for name, (_, ro, _) in runs.items():
            us[name].append(timed(ro.run, REPS) / N_STEPS)
    res = {"us_per_step": {k: statistics.median(v) for k, v in us.items()}, "spec": runs["plain"][0].spec_index}
    # ---- the relabel beside fwg_gae, on the last rollout's buffers
    vec, ro, log = runs["goal_log"]
    lib, mem, buf = vec._lib, vec._mem, ro.buf
    out = log.relabel(buf, p=0.8, seed=1)
    adv, ret = torch.empty_like(buf["rewards"]), torch.empty_like(buf["rewards"])
    calls = {"fwg_goal_relabel": lambda: log.relabel(buf, p=0.8, seed=1, out=out),
             "fwg_gae": lambda: gae(lib, mem, buf["rewards"], buf["values"], buf["dones"], ro.last_value, 0.99, 0.95, adv, ret)}
    W = goal_window(vec)
    M = N_STEPS * envs
    ach = log.achieved[1:].reshape(M, 4).contiguous()
    des = log.desired[:N_STEPS].reshape(M, 4).contiguous()
    win = torch.zeros((W, M, 4), device=ach.device)
    win[W - 1, :, :3] = buf["actions"].reshape(M, 3)
    step = (log.achieved[:N_STEPS, :, 3].contiguous().view(torch.int32) & 0xFFFF).reshape(M).contiguous()
    rew = torch.empty((M,), device=ach.device)
    spec = log.spec.struct(0)
    calls["fwg_goal_reward"] = lambda: nat.check(lib, lib.fwg_goal_reward(vec._handle, ctypes.byref(spec), M, mem.ptr(ach), mem.ptr(des), ctypes.c_void_p(),
                                                                          mem.ptr(win), mem.ptr(step), mem.ptr(rew), mem.stream()))
    for call in calls.values():
        for _ in range(K_WARM):
            call()
    torch.cuda.synchronize()
    k_us = {k: [] for k in calls}
    for _ in range(BLOCKS):
        for name, call in calls.items():
            k_us[name].append(timed(call, K_REPS))
    res["kernel_us"] = {k: statistics.median(v) for k, v in k_us.items()}
    src = out["src_row"]
    res["relabelled_share"] = float((src >= 0).sum()) / src.numel()
    res["window"] = W
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.envs)
    rows = []
    for _ in range(args.runs):                   # one process at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--child"], check=True, capture_output=True,
                           text=True, timeout=400)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    M = args.envs * N_STEPS
    share = statistics.median(r["relabelled_share"] for r in rows)
    relabel_bytes = M * (BYTES["scan"] + BYTES["reward_any"] + share * BYTES["reward_relabelled"])
    out = {"shape": "{} envs x {} steps, default preset with goals roll / pitch / Va".format(args.envs, N_STEPS),
           "method": "one fresh process per run, medians of {} runs; inside a run {} alternating blocks per figure, device events".format(args.runs, BLOCKS),
           "kernel_instance": rows[0]["spec"],
           "rollout_us_per_step": {k: spread([r["us_per_step"][k] for r in rows]) for k in ("plain", "goal_log")},
           "kernel_us": {k: spread([r["kernel_us"][k] for r in rows]) for k in ("fwg_goal_relabel", "fwg_gae", "fwg_goal_reward")},
           "relabelled_share": share, "window": rows[0]["window"], "bytes_per_transition": BYTES}
    out["rollout_us_per_step"]["difference"] = out["rollout_us_per_step"]["goal_log"]["median"] - out["rollout_us_per_step"]["plain"]["median"]
    out["algorithmic_GB_per_s"] = {
        "fwg_goal_relabel": relabel_bytes / (out["kernel_us"]["fwg_goal_relabel"]["median"] * 1e-6) / 1e9,
        "fwg_gae": M * BYTES["fwg_gae"] / (out["kernel_us"]["fwg_gae"]["median"] * 1e-6) / 1e9,
        "fwg_goal_reward": M * (BYTES["fwg_goal_reward"] + 16 * rows[0]["window"]) / (out["kernel_us"]["fwg_goal_reward"]["median"] * 1e-6) / 1e9}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
