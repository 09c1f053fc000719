#!/usr/bin/env python3
"""Times the collection of one exploration rollout for hindsight replay, per collected env step, on examples/train_her.py's
configuration at 4 096 and 65 536 envs x 64 steps -- three paths in one process:

  torch_loop_us       the example's eager loop (--collect torch): agent.act out of torch modules, three copies into rollout rows,
                      GoalVecEnv.step_device and GoalLog.observe around every fwg_step.  The BASELINE: the feature has no earlier
                      version, this is the loop the parent commit runs
  collector_eager_us  behaviour.HindsightCollector(graph=False): fwg_step + one fwg_behaviour_act per step, launched from Python
  collector_graph_us  HindsightCollector(graph=True): the same 2 T + 1 launches replayed as one graph
and beside them one launch alone, issued back to back:
  head_launch_us      fwg_behaviour_act with an env handle (goal rows, gather, observation copy, actor, exploration, stores)
  goal_observe_us     fwg_goal_observe (what the head's goal-row stage replaces)
  env_step_us         fwg_step under fixed actions
One fresh process per run, medians of `--runs` runs; inside a run two warm-up rollouts per path, then 5 alternating blocks of 3
rollouts (single launches: 200 per block), device events around each block.  A rollout's time includes the host's launch
cost wherever the device waits for the host: that is what a training run waits for.

    timeout -k 10 1100 python tools/time_collect.py --out profiles/collect_timing.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "examples")]

T = 64
SIZES = [4096, 65536]


def timed(call, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def child(sizes):
    import torch
    import train_her
    from gym_fixed_wing import goal
    from gym_fixed_wing.behaviour import HindsightCollector
    from gym_fixed_wing.goal import GoalLog, GoalVecEnv
    from gym_fixed_wing.offpolicy import DDPG
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    dev = torch.device("cuda", 0)
    out = {}
    for N in sizes:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            vecs = [FixedWingVecEnv(train_her.her_config(), num_envs=N, device=0, seed=0) for _ in range(3)]
        D = vecs[0].obs_dim
        agent = DDPG(D, 3, 3, update="hip", device=dev, seed=0)
        # ---- the example's loop, as it stands
        env, log = GoalVecEnv(vecs[0]), GoalLog(vecs[0], T)
        obs, actions = torch.zeros((T, N, D), device=dev), torch.zeros((T, N, 3), device=dev)
        raw, dones = torch.zeros((T, N), device=dev), torch.zeros((T, N), dtype=torch.uint8, device=dev)
        state = {"cur": env.reset()}

        def torch_loop():
            cur = state["cur"]
            log.observe(0)
            for t in range(T):
                a = agent.act(cur["observation"].reshape(N, D), cur["desired_goal"], noise=0.2)
                obs[t].copy_(cur["observation"].reshape(N, D))
                actions[t].copy_(a)
                cur, _, d = env.step_device(actions[t], reward_out=raw[t])
                dones[t].copy_(d)
                log.observe(t + 1)
            state["cur"] = cur
        # ---- the collector, eager and replayed
        vecs[1].reset(), vecs[2].reset()
        eager = HindsightCollector(vecs[1], agent, T, seed=0, noise=0.2)
        graphed = HindsightCollector(vecs[2], agent, T, graph=True, seed=0, noise=0.2)
        # ---- single launches (on the eager collector's env: launches only, the state does not matter)
        v, m = vecs[1], vecs[1]._mem
        spec = eager.goals.spec.struct(0)
        ach, des = m.zeros((N, 4)), m.zeros((N, 4))
        fixed = torch.zeros((N, 3), device=dev)
        calls = {"torch_loop_us": (torch_loop, 3, T), "collector_eager_us": (eager.run, 3, T), "collector_graph_us": (graphed.run, 3, T),
                 "head_launch_us": (lambda: eager._act(0, eager.cur, eager.buf["dones"][0]), 200, 1),
                 "goal_observe_us": (lambda: goal._observe(v, spec, ach, des), 200, 1),
                 "env_step_us": (lambda: v.step_device(fixed), 200, 1)}
        for call, _, _ in calls.values():
            for _ in range(2):
                call()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(5):   # alternating blocks
            for k, (call, reps, per) in calls.items():
                us[k].append(timed(call, reps) / per)
        out["N{}".format(N)] = {k: statistics.median(x) for k, x in us.items()}
        assert bool(torch.isfinite(graphed.buf["actions"]).all()) and bool(torch.isfinite(eager.buf["actions"]).all())
        graphed.head.close(), eager.head.close(), agent.close()
        vecs[2].set_graph_mode(False)
        del graphed, eager
        for x in vecs:
            x.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.sizes)
    rows = []
    for i in range(args.runs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes"] + [str(s) for s in args.sizes],
                           capture_output=True, text=True)
        if r.returncode != 0:   # (no second process is started on a card one has just failed on)
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("run {}: {}".format(i, r.stdout.strip().splitlines()[-1]), file=sys.stderr, flush=True)
    out = {"configuration": "examples/train_her.py her_config(), {} steps per rollout, DDPG(update='hip'), noise 0.2".format(T),
           "method": "one fresh process per run, medians of {} runs; inside a run two warm-up rollouts per path, then 5 alternating blocks of 3 "
                     "rollouts (single launches: 200 per block), device events; microseconds per collected env step (rollout time / {}), "
                     "single launches per launch".format(args.runs, T),
           "launches_per_rollout": {"collector": 2 * T + 1}, "cases": {}}
    for case in rows[0]:
        c = {k: {"median": statistics.median(r[case][k] for r in rows), "min": min(r[case][k] for r in rows), "max": max(r[case][k] for r in rows)}
             for k in rows[0][case]}
        c["torch_loop_over_collector_eager"] = c["torch_loop_us"]["median"] / c["collector_eager_us"]["median"]
        c["torch_loop_over_collector_graph"] = c["torch_loop_us"]["median"] / c["collector_graph_us"]["median"]
        out["cases"][case] = c
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    sys.exit(main())
