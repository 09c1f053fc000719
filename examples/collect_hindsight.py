#!/usr/bin/env python3
"""Hindsight experience replay's data path on MI355X, without the learner: rollouts of the `default` preset with the goals roll /
pitch / Va (the reference's FixedWingAircraftGoal, fixed_wing.py:1165-1277), one hipGraph per rollout with a goal row behind
every env step, and HER's "future" relabelling of the whole rollout in one call -- no host loop over transitions.

    python examples/collect_hindsight.py --envs 65536 --rollouts 5
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

import torch  # noqa: E402

from gym_fixed_wing import presets  # noqa: E402
from gym_fixed_wing.actor import DeviceActor  # noqa: E402
from gym_fixed_wing.goal import GoalLog  # noqa: E402
from gym_fixed_wing.rollout import FusedRollout, MlpPolicy  # noqa: E402
from gym_fixed_wing.vec_env import FixedWingVecEnv  # noqa: E402

GOALS = [{"name": "roll", "mean": 0.0, "var": 1.0}, {"name": "pitch", "mean": 0.0, "var": 0.5}, {"name": "Va", "mean": 22.0, "var": 10.0}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rollouts", type=int, default=5)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--p", type=float, default=0.8, help="share of the eligible transitions that take a future goal")
    args = ap.parse_args()
    cfg = presets.preset("default")
    cfg["observation"]["goals"] = GOALS
    vec = FixedWingVecEnv(cfg, num_envs=args.envs, device=0, seed=0)
    vec.reset()
    torch.manual_seed(0)
    actor = DeviceActor.for_env(vec, seed=1)
    actor.load_policy(MlpPolicy(vec.obs_dim))
    log = GoalLog(vec, args.n_steps)
    rollout = FusedRollout(vec, actor, args.n_steps, graph=True, raw_rewards=True, goals=log)
    out = None
    for it in range(args.rollouts):
        buf = rollout.run()                                  # ... + log.achieved / log.desired [n_steps + 1, N, 4]
        out = log.relabel(buf, p=args.p, seed=7, out=out)    # desired_goal [n_steps, N, 4], rewards, src_row
        # ... a replay buffer would store (obs, log.achieved, out["desired_goal"], actions, out["rewards"]) here ...
        src = out["src_row"]
        n = float(src.numel())
        print("rollout {:3d}: relabelled {:.3f}  kept {:.3f}  terminal {:.3f}  window before the rollout {:.3f}   mean reward raw {:+.4f} "
              "relabelled {:+.4f}".format(it, float((src >= 0).sum()) / n, float((src == -1).sum()) / n, float((src == -2).sum()) / n,
                                          float((src == -3).sum()) / n, float(buf["raw_rewards"].mean()), float(out["rewards"].mean())), flush=True)
    actor.close()
    vec.close()


if __name__ == "__main__":
    main()
