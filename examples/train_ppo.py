#!/usr/bin/env python3
"""Train a PPO attitude controller on the MI355X-native env -- the reference's examples/train_rl_controller.py
(`VecNormalize(SubprocVecEnv(...))` + `PPO2(MlpPolicy, env).learn(5e6, callback=monitor_training)` with the curriculum rule of
its callback, :80-87) with the whole data path on the device: rollouts by the HIP head + env step kernels, advantages by fwg_gae,
the PPO2 update in torch on the same buffers (or, with --update hip, as HIP kernels for either policy: gym_fixed_wing/learner.py), the success sums all-gathered over RCCL, the curriculum raised on every rank.

    python examples/train_ppo.py --envs 4096 --timesteps 100e6 --out model.npz
    python examples/train_ppo.py --policy cnn --envs 4096 --timesteps 100e6 --out cnn_model.npz   (the CNN controller)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_ppo.py --envs 32768

The reference trains 4 sub-process envs for 5 M steps (~8 h of PyFly on 4 cores; examples/tensorboard.png: success_all ~0.8 at
4-5 M steps).  4 096 device envs deliver 5 M steps in ten rollouts; a batch of 524 288 transitions per update learns less per
SAMPLE than 512 do, so the recipe below spends more samples (default 100 M, about a minute) with 128 minibatches per update and
twice the learning rate -- everything else is PPO2's defaults (gym_fixed_wing/ppo.py PPO2_DEFAULTS).  Measured (MI355X, seed 0):
curriculum level 1 after 58 M steps, success_all 0.79 at 74 M, 0.90 at 148 M (profiles/r06_ppo_training.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "fixed-wing-gym_amd")]

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gym_fixed_wing import presets  # noqa: E402
from gym_fixed_wing.distributed import CurriculumSchedule, make_sharded_env  # noqa: E402
from gym_fixed_wing.ppo import PPO, sb_init_  # noqa: E402
from gym_fixed_wing.rollout import CnnMlpPolicy  # noqa: E402


def train(envs=4096, timesteps=100e6, seed=0, nminibatches=128, noptepochs=4, learning_rate=5e-4, n_steps=128, curriculum=True,
          config=None, log=print, rank=0, world=1, local=0, fused=None, ent_coef=0.01, on_update=None, update="torch", policy="mlp",
          test_set=None, test_turbulence="none", render_dir=None, render_every=600.0, monitor=False, log_dir=None, log_interval=50,
          checkpoint_every=None, checkpoint_path=None):
    """policy: "mlp" (MlpPolicy on the examples config's 12-vector) or "cnn" (CnnMlpPolicy on the cnn config's 5 x 12 matrix
    observations: the reference's --policy CNN, train_rl_controller.py:179-197).  update: "torch" or "hip" (for the cnn policy
    "hip" is PPO's "hip_cnn").  config: preset name, default by policy.
    test_set: a list of scenarios (or the path of one as JSON, the format of examples/evaluate_controller.py): rank 0 flies it
    with the current policy whenever num_timesteps crosses a fifth of `timesteps` -- the reference's test_interval =
    training_steps / 5 (train_rl_controller.py --test-set-path), four evaluations in a run -- by PPO.evaluate (the evaluation
    protocol on the device); the table goes into that update's info["test"].
    render_dir: rank 0 records env 0 on the device (gym_fixed_wing.recorder.FlightRecorder) and, whenever `render_every` seconds
    have passed and env 0 has finished another episode, saves that episode's figure as <render_dir>/<num_timesteps>.png -- the
    reference's render_interval = 600 s of training episodes (train_rl_controller.py:95-104).
    monitor: PPO(monitor=True) -- every info carries the finished episodes' mean return and length (stable-baselines' ep_rewmean /
    eplenmean, gym_fixed_wing.monitor) and all five info_kw measures per target state (info["ep_info"]).
    log_dir: rank 0 appends every update's info to <log_dir>/progress.csv and prints the reference's block of the five measures
    every `log_interval` updates (monitor.ProgressLog; the first job of the reference's monitor_training).
    checkpoint_every: rank 0 saves the model to `checkpoint_path` whenever that many seconds have passed (the reference's
    save_interval = 300 s)."""
    if isinstance(test_set, str):
        with open(test_set) as f:
            test_set = json.load(f)
    config = config or ("cnn" if policy == "cnn" else "examples")
    # (the cnn configuration's build-time kernel instance is the shipped one, derived views on: presets.SPECIALISED ship_cnn_log)
    vec = make_sharded_env(presets.preset(config), total_envs=envs, rank=rank, world_size=world, device=local,
                           derived_views=config == "cnn", seed=seed)
    recorder = None
    if render_dir is not None and rank == 0:
        # before the first reset (an episode is recorded from its reset on) and before PPO captures its rollout (a graph captured
        # earlier would replay without the recorder's launches)
        from gym_fixed_wing.recorder import FlightRecorder
        recorder = FlightRecorder(vec, env_ids=(0,))
    sched = CurriculumSchedule(level=0.25 if curriculum else 1.0)     # (train_rl_controller.py:162: curriculum_level = 0.25)
    vec.set_curriculum_level(sched.level)
    vec.reset()
    net = None
    if policy == "cnn":
        torch.manual_seed(seed)
        net = sb_init_(CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3))
    if policy == "cnn" and update == "hip":
        update = "hip_cnn"
    ppo = PPO(vec, policy=net, seed=seed, curriculum=sched, n_steps=n_steps, nminibatches=nminibatches, noptepochs=noptepochs,
              learning_rate=learning_rate, fused=fused, ent_coef=ent_coef, update=update, monitor=monitor)
    t0 = time.perf_counter()
    progress = None
    if log_dir is not None and rank == 0:
        from gym_fixed_wing.monitor import ProgressLog
        progress = ProgressLog(log_dir, log_interval, out=log)
    saved = {"at": t0, "files": 0}
    window = []    # success over the last finished episodes (the reference's ep_info_buf holds the last 100)
    tests_done = [0]
    rendered = {"at": t0, "episodes": 0, "files": []}

    def on_info(info):
        if recorder is not None and time.perf_counter() - rendered["at"] >= render_every:
            n_done = recorder.completed(0)
            if n_done > rendered["episodes"]:
                path = os.path.join(render_dir, "{}.png".format(int(info["timesteps"])))
                recorder.render(mode="plot", show=False, save_path=path)
                rendered.update(at=time.perf_counter(), episodes=n_done)
                rendered["files"].append(path)
                if log is not None:
                    log("update {:4d}  rendered episode {} of env 0 -> {}".format(info["update"], n_done, path))
        fifth = int(info["timesteps"] // (timesteps / 5.0))
        if test_set is not None and rank == 0 and min(fifth, 4) > tests_done[0]:
            tests_done[0] = min(fifth, 4)
            info["test"] = ppo.evaluate(test_set, turbulence_intensity=test_turbulence)
            if log is not None:
                t = info["test"]
                log("update {:4d}  test set ({} scenarios, turbulence {}): success_all {:.1f} %  settling {}  control variation {:.3f}".format(
                    info["update"], len(test_set), test_turbulence, t["success_%"]["all"],
                    " ".join("{} {:.2f} s".format(k, v) for k, v in t["settling_time"].items()), t["control_variation"]["all"]))
        if info["episodes"] > 0:
            window.append((info["episodes"], info["success"]["all"], info["level"]))
        if rank == 0 and log is not None and (info["episodes"] > 0 or info["update"] % 20 == 0):
            ep = ""
            if info.get("ep_rew_mean") is not None:
                ep = "  ep_rew {:+.3f}  ep_len {:.1f}".format(info["ep_rew_mean"], info["ep_len_mean"])
            log("update {:4d}  steps {:10.3e}  level {:.2f}  episodes {:6d}  success_all {}  pg {:+.4f}  vf {:.4f}  kl {:.4f}  std-entropy {:+.2f}  {:.0f} s{}".format(
                info["update"], info["timesteps"], info["level"], info["episodes"],
                "{:.3f}".format(info["success"]["all"]) if info["episodes"] else "  -  ", info["pg_loss"], info["vf_loss"], info["approx_kl"],
                info["entropy"], time.perf_counter() - t0, ep))
        if progress is not None:
            progress(info)
        if checkpoint_every is not None and checkpoint_path and rank == 0 and time.perf_counter() - saved["at"] >= checkpoint_every:
            ppo.save(checkpoint_path)
            saved.update(at=time.perf_counter(), files=saved["files"] + 1)
        if on_update is not None:
            on_update(ppo, info)

    ppo.learn(timesteps, log=on_info)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return ppo, {"seconds": dt, "env_steps_per_s": ppo.num_timesteps / dt, "updates": ppo.updates, "episodes_log": window,
                 "rendered": rendered["files"], "checkpoints": saved["files"],
                 "progress": None if progress is None else progress.path}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096, help="total over all ranks")
    ap.add_argument("--timesteps", type=float, default=100e6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nminibatches", type=int, default=128)
    ap.add_argument("--noptepochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    ap.add_argument("--disable-curriculum", action="store_true")
    ap.add_argument("--update", choices=("torch", "hip"), default="torch", help="PPO update: torch autograd (default) or the HIP kernels")
    ap.add_argument("--policy", choices=("mlp", "cnn"), default="mlp",
                    help="mlp: MlpPolicy, examples config; cnn: CnnMlpPolicy (3 filters), cnn config (either update)")
    ap.add_argument("--test-set", default=None, help="scenarios (JSON) flown with the current policy at every fifth of --timesteps (rank 0)")
    ap.add_argument("--test-turbulence", default="none", choices=["none", "light", "moderate", "severe"])
    ap.add_argument("--render-dir", default=None, help="save the figure of a training episode of env 0 as DIR/<num_timesteps>.png (rank 0)")
    ap.add_argument("--render-every", type=float, default=600.0, help="seconds between two rendered episodes (the reference's interval)")
    ap.add_argument("--log-dir", default=None, help="append every update to DIR/progress.csv and print the per-state measures (rank 0)")
    ap.add_argument("--log-interval", type=int, default=50, help="updates between two printed blocks of the per-state measures")
    ap.add_argument("--checkpoint-every", type=float, default=None, metavar="SECONDS",
                    help="save to --out whenever that many seconds have passed (the reference saves every 300 s; rank 0)")
    ap.add_argument("--out", default=None, help="save weights + VecNormalize statistics (.npz)")
    ap.add_argument("--curve", default=None, help="write the learning curve (JSON)")
    args = ap.parse_args()
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    ppo, res = train(args.envs, args.timesteps, args.seed, args.nminibatches, args.noptepochs, args.lr, curriculum=not args.disable_curriculum,
                     rank=rank, world=world, local=local, ent_coef=args.ent_coef, update=args.update, policy=args.policy,
                     test_set=args.test_set, test_turbulence=args.test_turbulence, render_dir=args.render_dir,
                     render_every=args.render_every, monitor=True, log_dir=args.log_dir, log_interval=args.log_interval,
                     checkpoint_every=args.checkpoint_every, checkpoint_path=args.out)
    if rank == 0:
        print("{:.3e} env-steps in {:.1f} s = {:.3e} env-steps/s INCLUDING the optimiser ({} updates)".format(
            ppo.num_timesteps, res["seconds"], res["env_steps_per_s"], res["updates"]))
        if args.out:
            ppo.save(args.out)
        if args.curve:
            with open(args.curve, "w") as f:
                json.dump({"args": vars(args), "history": ppo.history, **{k: v for k, v in res.items()}}, f)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
