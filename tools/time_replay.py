#!/usr/bin/env python3
"""What the device hindsight replay buffer (gym_fixed_wing.replay) costs, at 65 536 envs x 128 steps on the `default` preset with the
goals roll / pitch / Va, 4 slots, strategy "future", p = 0.8:

  1. fwg_replay_index per slot (one launch over dones [128][65536]);
  2. fwg_replay_sample at B = 65 536 and B = 1 048 576, as us and as the bandwidth its own algorithmic byte count comes to: per
     sample 2 * 4 D + 12 + 3 * 16 + 12 W + 13 bytes read (two observation rows, the action, three goal rows, the action window,
     raw reward + done + ep_end) and 2 * 4 D + 12 + 32 + 4 + 1 + 16 written; and the same count with every random read rounded up
     to whole 128-byte lines, which is what the memory system moves;
  3. the yardstick, in the same process: torch advanced indexing with the SAME (k, t, n) on the SAME buffers -- seven gathers
     (observation, next observation, action, raw reward, done, achieved goal, desired goal) -- and, at B = 1 048 576, one
     fwg_goal_reward call on the gathered rows on top (its action window rows are not gathered: the yardstick is let off that).
     The yardstick draws no goal and does no relabelling; it is the floor of a host-driven buffer, not the code under test.

Every run is one process of its own (construction, the rollouts that fill the slots and warm-up not timed); the figures are the
medians of 5 such runs.

    python tools/time_replay.py [--out profiles/replay_timing.json] [--envs 65536] [--runs 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]
N_STEPS, SLOTS, P = 128, 4, 0.8
K_WARM, K_REPS, BLOCKS = 5, 20, 3
BATCHES = (65536, 1048576)
GOALS = [{"name": "roll", "mean": 0.0, "var": 1.0}, {"name": "pitch", "mean": 0.0, "var": 0.5}, {"name": "Va", "mean": 22.0, "var": 10.0}]
LINE = 128


def bytes_per_sample(D, W):
    lines = lambda b: -(-b // LINE) * LINE
    read = 2 * 4 * D + 12 + 3 * 16 + 12 * W + 13
    written = 2 * 4 * D + 12 + 32 + 4 + 1 + 16
    read_lines = 2 * lines(4 * D) + LINE + 3 * LINE + W * LINE + 3 * LINE   # (a row that straddles a line boundary costs one more)
    return {"read": read, "written": written, "read_in_whole_lines": read_lines}


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
    from gym_fixed_wing.replay import HindsightReplay
    from gym_fixed_wing.rollout import FusedRollout, MlpPolicy
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    cfg = presets.preset("default")
    cfg["observation"]["goals"] = GOALS
    vec = FixedWingVecEnv(cfg, num_envs=envs, device=0, seed=1)
    vec.reset()
    actor = DeviceActor.for_env(vec, seed=3)
    torch.manual_seed(0)
    actor.load_policy(MlpPolicy(vec.obs_dim))
    log = GoalLog(vec, N_STEPS)
    ro = FusedRollout(vec, actor, N_STEPS, graph=True, raw_rewards=True, goals=log)
    replay = HindsightReplay(vec, N_STEPS, SLOTS, strategy="future", p=P, seed=1, target_observations="stale")
    for _ in range(SLOTS):
        ro.run()
        replay.add_rollout(ro)
    lib, mem = vec._lib, vec._mem
    W, D = goal_window(vec), replay.obs_dim
    calls = {"fwg_replay_index": lambda: nat.check(lib, lib.fwg_replay_index(N_STEPS, envs, mem.ptr(replay.dones[0]), mem.ptr(replay.ep_end[0]), mem.stream()))}
    share = {}
    for B in BATCHES:
        out = replay.sample(B)
        share[B] = float((out["index"][:, 3] >= 0).sum()) / B
        k, t, n = (out["index"][:, i].long() for i in range(3))
        calls["fwg_replay_sample_{}".format(B)] = lambda B=B, out=out: replay.sample(B, out=out)

        def gathers(k=k, t=t, n=n):
            return (replay.obs[k, t, n], replay.obs[k, t + 1, n], replay.actions[k, t, n], replay.raw_rewards[k, t, n], replay.dones[k, t, n],
                    replay.achieved[k, t + 1, n], replay.desired[k, t, n])
        calls["torch_gathers_{}".format(B)] = gathers
        if B == BATCHES[-1]:
            win, rew = torch.zeros((W, B, 4), device=out["reward"].device), torch.empty((B,), device=out["reward"].device)
            step = torch.zeros((B,), dtype=torch.int32, device=rew.device)
            spec = replay.spec.struct(1)

            def gathers_and_reward(k=k, t=t, n=n, B=B):
                g = gathers(k, t, n)
                nat.check(lib, lib.fwg_goal_reward(vec._handle, ctypes.byref(spec), B, mem.ptr(g[5]), mem.ptr(g[6]), ctypes.c_void_p(), mem.ptr(win),
                                                   mem.ptr(step), mem.ptr(rew), mem.stream()))
                return g
            calls["torch_gathers_and_goal_reward_{}".format(B)] = gathers_and_reward
    for call in calls.values():
        for _ in range(K_WARM):
            call()
    torch.cuda.synchronize()
    us = {name: [] for name in calls}
    for _ in range(BLOCKS):                      # alternating blocks
        for name, call in calls.items():
            us[name].append(timed(call, K_REPS))
    print(json.dumps({"us": {k: statistics.median(v) for k, v in us.items()}, "relabelled_share": {str(b): s for b, s in share.items()},
                      "window": W, "obs_words": D, "spec": vec.spec_index}))
    actor.close()
    vec.close()


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
    for _ in range(args.runs):                   # one process at a time; a run that fails or hangs ends the measurement
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--child"], check=True, capture_output=True,
                           text=True, timeout=300)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}

    W, D = rows[0]["window"], rows[0]["obs_words"]
    per = bytes_per_sample(D, W)
    out = {"shape": "{} envs x {} steps x {} slots, default preset with goals roll / pitch / Va, strategy future, p {}".format(args.envs, N_STEPS, SLOTS, P),
           "method": "one fresh process per run, medians of {} runs; inside a run {} alternating blocks of {} calls per figure, device events".format(
               args.runs, BLOCKS, K_REPS),
           "kernel_instance": rows[0]["spec"], "window": W, "obs_words": D, "bytes_per_sample": per,
           "relabelled_share": {b: statistics.median(r["relabelled_share"][b] for r in rows) for b in rows[0]["relabelled_share"]},
           "us": {k: spread([r["us"][k] for r in rows]) for k in rows[0]["us"]}}
    out["fwg_replay_index_GB_per_s"] = args.envs * N_STEPS * 5 / (out["us"]["fwg_replay_index"]["median"] * 1e-6) / 1e9   # 1 B read, 4 B written
    out["fwg_replay_sample_GB_per_s"] = {}
    for B in BATCHES:
        sec = out["us"]["fwg_replay_sample_{}".format(B)]["median"] * 1e-6
        out["fwg_replay_sample_GB_per_s"][str(B)] = {"algorithmic": B * (per["read"] + per["written"]) / sec / 1e9,
                                                     "reads_in_whole_lines": B * (per["read_in_whole_lines"] + per["written"]) / sec / 1e9}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
