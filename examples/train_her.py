#!/usr/bin/env python3
"""Hindsight experience replay with an off-policy learner on MI355X: gym_fixed_wing.offpolicy.DDPG over the device replay buffer
(gym_fixed_wing.replay.HindsightReplay); --update hip runs the update as HIP kernels, --twin / --policy-delay 2 make it TD3-style.
The env is the `default` preset with the goals roll / pitch / Va (the reference's FixedWingAircraftGoal) and WITHOUT the goal
states' target entries in the observation vector -- the goal reaches the networks as `desired_goal` only, so a relabelled sample is
consistent (that configuration is no build-time preset: at 1 024 envs or more a specialised kernel is compiled for it once).
Per iteration: n_steps behaviour steps of every env with Gaussian exploration, one
replay.add, then updates on minibatches that replay.sample relabels while it draws them -- no host loop over transitions.

    python examples/train_her.py --envs 4096 --iters 30 --n-steps 64 --batch 4096 --strategy future
    python examples/train_her.py --update hip --twin --policy-delay 2

It shows the buffer in use; it is no tuned controller."""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

import torch  # noqa: E402

from gym_fixed_wing import presets  # noqa: E402
from gym_fixed_wing.goal import GoalLog, GoalVecEnv  # noqa: E402
from gym_fixed_wing.offpolicy import DDPG  # noqa: E402
from gym_fixed_wing.replay import HindsightReplay, without_goal_targets  # noqa: E402
from gym_fixed_wing.vec_env import FixedWingVecEnv  # noqa: E402

GOALS = [{"name": "roll", "mean": 0.0, "var": 1.0}, {"name": "pitch", "mean": 0.0, "var": 0.5}, {"name": "Va", "mean": 22.0, "var": 10.0}]


def her_config():
    cfg = presets.preset("default")
    cfg["observation"]["goals"] = copy.deepcopy(GOALS)
    return without_goal_targets(cfg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--n-steps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--strategy", default="future", choices=["future", "final", "episode"])
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--updates", type=int, default=40, help="minibatch updates per iteration")
    ap.add_argument("--p", type=float, default=0.8, help="share of the eligible samples that take a hindsight goal")
    ap.add_argument("--noise", type=float, default=0.2, help="std of the Gaussian exploration noise")
    ap.add_argument("--gamma", type=float, default=0.98)
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--update", default="torch", choices=["torch", "hip"], help="the update path: torch autograd, or the HIP kernels")
    ap.add_argument("--twin", action="store_true", help="two critics, the target takes the smaller value (TD3's clipped double-Q)")
    ap.add_argument("--policy-delay", type=int, default=1, help="critic updates per actor update (TD3: 2)")
    ap.add_argument("--collect", default="torch", choices=["torch", "device"],
                    help="the behaviour rollout: the torch loop below, or gym_fixed_wing.behaviour.HindsightCollector (one HIP launch per act)")
    ap.add_argument("--graph", action="store_true", help="--collect device: capture the rollout once and replay it (--n-steps must be even)")
    ap.add_argument("--random-eps", type=float, default=0.0, help="--collect device: probability of a uniform random action per env and step")
    args = ap.parse_args()
    if args.graph and args.collect != "device":
        ap.error("--graph needs --collect device")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vec = FixedWingVecEnv(her_config(), num_envs=args.envs, device=0, seed=0)
    env = GoalVecEnv(vec)
    T, N, D, G = args.n_steps, args.envs, vec.obs_dim, env.spec.n
    log = GoalLog(vec, T)
    replay = HindsightReplay(vec, T, args.slots, strategy=args.strategy, p=args.p, seed=1)
    agent = DDPG(D, G, 3, n_critics=2 if args.twin else 1, gamma=args.gamma, tau=args.tau, lr_actor=args.lr, lr_critic=args.lr,
                 policy_delay=args.policy_delay, update=args.update, device=dev)
    # the behaviour rollout, step-major, as replay.add takes it
    obs = torch.zeros((T, N, D), device=dev)
    actions, raw = torch.zeros((T, N, 3), device=dev), torch.zeros((T, N), device=dev)
    dones = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    cur = env.reset()
    collector = None
    if args.collect == "device":   # the same rollout as 2 T + 1 launches (with --graph: one replayed graph)
        from gym_fixed_wing.behaviour import HindsightCollector
        collector = HindsightCollector(vec, agent, T, graph=args.graph, seed=0, noise=args.noise, random_eps=args.random_eps)
        log, raw = collector.goals, collector.buf["raw_rewards"]
    batch = None
    for it in range(args.iters):
        if collector is not None:
            collector.head.refresh()   # (--update torch: the head acts on a copy of the actor's weights)
            collector.run()
            replay.add_rollout(collector)
        else:
            log.observe(0)
            for t in range(T):
                a = agent.act(cur["observation"].reshape(N, D), cur["desired_goal"], noise=args.noise)
                obs[t].copy_(cur["observation"].reshape(N, D))
                actions[t].copy_(a)
                cur, _, d = env.step_device(actions[t], reward_out=raw[t])
                dones[t].copy_(d)
                log.observe(t + 1)
            replay.add(obs, cur["observation"].reshape(N, D), actions, raw, dones, log)
        # the final distance to the goal of the rollout's last row, in scaled units
        miss = (log.achieved[T, :, :G] - log.desired[T, :, :G]).abs().mean(dim=0)
        stats = {"critic_loss": 0.0, "actor_loss": 0.0}
        relabelled = 0.0
        for _ in range(args.updates):
            batch = replay.sample(args.batch, out=batch)
            stats = agent.update(batch)
            relabelled = float((batch["index"][:, 3] >= 0).float().mean())
        print("iter {:3d}  critic_loss= {:.5f}  actor_loss= {:+.5f}  step_reward= {:+.4f}  relabelled= {:.3f}  goal_miss= {}  stored= {}".format(
            it, stats["critic_loss"], stats["actor_loss"], float(raw.mean()), relabelled, " ".join("{:.3f}".format(float(x)) for x in miss), len(replay)), flush=True)
    vec.close()


if __name__ == "__main__":
    main()
