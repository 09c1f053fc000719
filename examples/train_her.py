#!/usr/bin/env python3
"""Hindsight experience replay with an off-policy learner on MI355X: a deliberately small DDPG in torch over the device replay
buffer (gym_fixed_wing.replay.HindsightReplay).  The env is the `default` preset with the goals roll / pitch / Va (the reference's
FixedWingAircraftGoal) and WITHOUT the goal states' target entries in the observation vector -- the goal reaches the networks as
`desired_goal` only, so a relabelled sample is consistent (that configuration is no build-time preset: at 1 024 envs or more a
specialised kernel is compiled for it once).  Per iteration: n_steps behaviour steps of every env with Gaussian exploration, one
replay.add, then updates on minibatches that replay.sample relabels while it draws them -- no host loop over transitions.

    python examples/train_her.py --envs 4096 --iters 30 --n-steps 64 --batch 4096 --strategy future

It shows the buffer in use; it is no tuned controller."""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

import torch  # noqa: E402
from torch import nn  # noqa: E402

from gym_fixed_wing import presets  # noqa: E402
from gym_fixed_wing.goal import GoalLog, GoalVecEnv  # noqa: E402
from gym_fixed_wing.replay import HindsightReplay, without_goal_targets  # noqa: E402
from gym_fixed_wing.vec_env import FixedWingVecEnv  # noqa: E402

GOALS = [{"name": "roll", "mean": 0.0, "var": 1.0}, {"name": "pitch", "mean": 0.0, "var": 0.5}, {"name": "Va", "mean": 22.0, "var": 10.0}]


def her_config():
    cfg = presets.preset("default")
    cfg["observation"]["goals"] = copy.deepcopy(GOALS)
    return without_goal_targets(cfg)


def mlp(n_in, n_out, hidden=64, out_act=None):
    layers = [nn.Linear(n_in, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, n_out)]
    return nn.Sequential(*(layers + ([out_act] if out_act is not None else [])))


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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vec = FixedWingVecEnv(her_config(), num_envs=args.envs, device=0, seed=0)
    env = GoalVecEnv(vec)
    T, N, D, G = args.n_steps, args.envs, vec.obs_dim, env.spec.n
    log = GoalLog(vec, T)
    replay = HindsightReplay(vec, T, args.slots, strategy=args.strategy, p=args.p, seed=1)
    actor, critic = mlp(D + G, 3, out_act=nn.Tanh()).to(dev), mlp(D + G + 3, 1).to(dev)
    actor_t, critic_t = copy.deepcopy(actor), copy.deepcopy(critic)
    opt_a, opt_c = torch.optim.Adam(actor.parameters(), lr=args.lr), torch.optim.Adam(critic.parameters(), lr=args.lr)
    # the behaviour rollout, step-major, as replay.add takes it
    obs = torch.zeros((T, N, D), device=dev)
    actions, raw = torch.zeros((T, N, 3), device=dev), torch.zeros((T, N), device=dev)
    dones = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    cur = env.reset()
    batch = None
    for it in range(args.iters):
        log.observe(0)
        for t in range(T):
            with torch.no_grad():
                a = actor(torch.cat([cur["observation"].reshape(N, D), cur["desired_goal"]], dim=1))
                a = (a + args.noise * torch.randn_like(a)).clamp(-1.0, 1.0)
            obs[t].copy_(cur["observation"].reshape(N, D))
            actions[t].copy_(a)
            cur, _, d = env.step_device(actions[t], reward_out=raw[t])
            dones[t].copy_(d)
            log.observe(t + 1)
        replay.add(obs, cur["observation"].reshape(N, D), actions, raw, dones, log)
        # the final distance to the goal of the rollout's last row, in scaled units
        miss = (log.achieved[T, :, :G] - log.desired[T, :, :G]).abs().mean(dim=0)
        loss_c = loss_a = torch.zeros((), device=dev)
        relabelled = 0.0
        for _ in range(args.updates):
            batch = replay.sample(args.batch, out=batch)
            o, g, a, r = batch["observation"], batch["desired_goal"], batch["action"], batch["reward"]
            o2, live = batch["next_observation"], 1.0 - batch["done"].float()
            with torch.no_grad():
                q2 = critic_t(torch.cat([o2, g, actor_t(torch.cat([o2, g], dim=1))], dim=1)).squeeze(1)
                target = r + args.gamma * live * q2      # (a terminal sample's next observation is the next episode's: masked)
            loss_c = ((critic(torch.cat([o, g, a], dim=1)).squeeze(1) - target) ** 2).mean()
            opt_c.zero_grad()
            loss_c.backward()
            opt_c.step()
            loss_a = -critic(torch.cat([o, g, actor(torch.cat([o, g], dim=1))], dim=1)).mean()
            opt_a.zero_grad()
            loss_a.backward()
            opt_a.step()
            with torch.no_grad():
                for net, tgt in ((actor, actor_t), (critic, critic_t)):
                    for p_, pt in zip(net.parameters(), tgt.parameters()):
                        pt.lerp_(p_, args.tau)
            relabelled = float((batch["index"][:, 3] >= 0).float().mean())
        print("iter {:3d}  critic_loss= {:.5f}  actor_loss= {:+.5f}  step_reward= {:+.4f}  relabelled= {:.3f}  goal_miss= {}  stored= {}".format(
            it, float(loss_c.detach()), float(loss_a.detach()), float(raw.mean()), relabelled, " ".join("{:.3f}".format(float(x)) for x in miss), len(replay)), flush=True)
    vec.close()


if __name__ == "__main__":
    main()
