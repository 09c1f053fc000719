"""PPO learner on top of the device-resident rollout (second half): what the reference's training
script does with `PPO2(MlpPolicy, VecNormalize(SubprocVecEnv(...))).learn(total_timesteps, callback=monitor_training)`
(examples/train_rl_controller.py:223-232; curriculum callback :80-87), with every env-side piece on the MI355X:

  rollout     FusedRollout: env step + VecNormalize + 64-64 MlpPolicy + sampling as HIP kernels (one or two launches per
              step), writing obs / actions / values / log-probs / normalised rewards / dones step-major in place;
  advantages  fwg_gae (HIP, one launch over the rollout buffers, 17 B per transition);
  update      the clipped-surrogate objective of stable-baselines' PPO2 with its defaults (gamma 0.99, lambda 0.95, clip 0.2 on
              policy AND value, entropy 0.01, value 0.5, lr 2.5e-4 Adam eps 1e-5, 4 epochs x 4 minibatches, gradient norm 0.5) --
              by one of learner.py's two updaters, which share one update() interface: TorchUpdater (the default) is torch
              autograd on the 12-64-64 networks (or the CnnMlpPolicy: conv + 36-64-64), each minibatch step one captured graph;
              HipLearner (PPO(update="hip"); "hip_cnn" for a CnnMlpPolicy) runs them as HIP kernels (forward / backward on the
              matrix cores, the conv on the VALU, clip and Adam on the device, one captured graph per update, the head repacked
              on the device);
  curriculum  distributed.gather_success (one RCCL all-gather of 64 B per rank) + CurriculumSchedule after every rollout;
  monitor     PPO(monitor=True): monitor.EpisodeMonitor -- the rollout keeps the raw rewards (written by the step kernel itself),
              fwg_monitor_fold folds them once per rollout, and learn() reports the episodes' mean return and length (PPO2's
              ep_rewmean / eplenmean) and all five info_kw measures per target state.

PPO is the training loop and the policy of an update (hyper-parameters, permutations, minibatch split); a step's mechanics are
the updater's (PPO.learner).  The torch policy is the master copy of the weights; the updater leaves them in the HIP head after
every update (DeviceActor.load_policy; with update="hip" / "hip_cnn" the parameters are views of the learner's flat device buffer and the head
is repacked on the device).  Multi-GPU: every rank collects its shard; gradients are averaged with one all-reduce per minibatch
step when torch.distributed is initialised (data-parallel PPO)."""
import math

import numpy as np
import torch
from torch import nn

from . import _native as nat
from .learner import STAT_KEYS, HipLearner, TorchUpdater, ppo_loss  # noqa: F401  (STAT_KEYS, ppo_loss: re-exported)
from .rollout import FusedRollout, MlpPolicy

# stable-baselines PPO2.__init__ defaults (the reference passes none: `PPO2(policy, env, verbose=1, tensorboard_log=...)`)
PPO2_DEFAULTS = dict(gamma=0.99, n_steps=128, ent_coef=0.01, learning_rate=2.5e-4, vf_coef=0.5, max_grad_norm=0.5, lam=0.95,
                     nminibatches=4, noptepochs=4, cliprange=0.2)


def sb_init_(policy):
    """stable-baselines' MlpPolicy initialisation: orthogonal, gain sqrt(2) on the hidden layers, 0.01 on the action mean,
    1 on the value output; zero biases; log-std 0 (common/policies.py mlp_extractor / linear(init_scale)).  A CnnMlpPolicy's
    conv: orthogonal over its [rows][n_filters] kernel (SB2's conv helper: ortho_init of the kernel flattened to [rows x 1 x 1]
    [n_filters]), zero bias, gain sqrt(2) -- the gain SB2's own CNN extractor (nature_cnn) passes; the fork's is not recorded."""
    conv = getattr(policy, "conv", None)
    if conv is not None:
        nn.init.orthogonal_(conv.weight, gain=math.sqrt(2.0))
        nn.init.zeros_(conv.bias)
    for net, out_gain in ((policy.pi, 0.01), (policy.vf, 1.0)):
        lin = [m for m in net if isinstance(m, nn.Linear)]
        for i, m in enumerate(lin):
            nn.init.orthogonal_(m.weight, gain=out_gain if i == len(lin) - 1 else math.sqrt(2.0))
            nn.init.zeros_(m.bias)
    with torch.no_grad():
        policy.log_std.zero_()
    return policy


def gae(lib, mem, rewards, values, dones, last_value, gamma, lam, adv_out=None, ret_out=None):
    """fwg_gae on buffers of the env's memory backend ([T, N] step-major; device tensors on the GPU)."""
    import ctypes
    T, N = int(rewards.shape[0]), int(rewards.shape[1])
    adv_out = mem.zeros((T, N)) if adv_out is None else adv_out
    ret_out = mem.zeros((T, N)) if ret_out is None else ret_out
    nat.check(lib, lib.fwg_gae(T, N, mem.ptr(rewards), mem.ptr(values), mem.ptr(dones), mem.ptr(last_value),
                               ctypes.c_float(gamma), ctypes.c_float(lam), mem.ptr(adv_out), mem.ptr(ret_out), mem.stream()))
    return adv_out, ret_out


def _blank(summary):
    """A gather_success summary with every mean None (no episode ended: the means would be 0 / 0)."""
    return {k: ({s: None for s in v} if isinstance(v, dict) else v) for k, v in summary.items()}


class PPO(object):
    """PPO2-style learner for a FixedWingVecEnv: MlpPolicy on the (flattened) observation by default, or
    policy=CnnMlpPolicy(...) on 5 x 12 matrix observations (train_rl_controller.py --policy CNN; update="torch" or "hip_cnn").  `learn(total_timesteps)` alternates
    rollouts of n_steps x num_envs transitions with noptepochs x nminibatches gradient steps; `callback(self, info)` runs after
    every update (the reference's monitor_training).  monitor=True: the rollout keeps its raw rewards, collect() folds them
    (monitor.EpisodeMonitor) and learn() adds the episodes' return / length statistics and info["ep_info"] to every info."""

    def __init__(self, vec, policy=None, seed=0, fused=None, graph=True, curriculum=None, group=None, precise=True,
                 graph_update=True, update="torch", monitor=False, **kw):
        from .actor import DeviceActor
        hp = dict(PPO2_DEFAULTS)
        unknown = set(kw) - set(hp)
        if unknown:
            raise TypeError("unknown PPO hyper-parameters: {}".format(sorted(unknown)))
        hp.update(kw)
        # ("hip_cnn" is a name of its own only because tests/test_cnn_policy.py pins that update="hip" refuses a policy with a conv;
        # a later change may merge the two into "hip")
        if update not in ("torch", "hip", "hip_cnn"):
            raise ValueError("update must be 'torch', 'hip' or 'hip_cnn', not {!r}".format(update))
        if update == "hip" and getattr(policy, "conv", None) is not None:
            raise ValueError("PPO(update='hip') is the MlpPolicy's update; for the conv of a CnnMlpPolicy use update='hip_cnn' (or 'torch')")
        if update == "hip_cnn" and getattr(policy, "conv", None) is None:
            raise ValueError("PPO(update='hip_cnn') needs a policy with a conv (CnnMlpPolicy); an MlpPolicy takes update='hip'")
        self.hp, self.vec, self.group = hp, vec, group
        self.n_steps = int(hp["n_steps"])
        self._torch_dev = getattr(vec._mem, "device", torch.device("cpu"))
        torch.manual_seed(seed)
        self.policy = (sb_init_(MlpPolicy(vec.obs_dim)) if policy is None else policy).to(self._torch_dev)
        self.actor = DeviceActor.for_env(vec, seed=seed, gamma=hp["gamma"], precise=precise)
        self.actor.load_policy(self.policy)
        self._rollout_kw = dict(graph=bool(graph) and self._torch_dev.type == "cuda", fused=fused)
        self.monitor = None
        if monitor:
            from .monitor import EpisodeMonitor
            self.monitor = EpisodeMonitor(vec)
            self._rollout_kw["raw_rewards"] = True   # (in the dictionary: the rollout built anew after a curriculum change keeps them)
        self._build_rollout()
        if update in ("hip", "hip_cnn"):   # (the module's parameters become views of its flat buffer here, before the broadcast below writes through them)
            self.learner = HipLearner(vec._lib, self.actor, self.policy, self._torch_dev, graph=graph_update, lr=hp["learning_rate"])
        else:
            self.learner = TorchUpdater(self.actor, self.policy, self._torch_dev, graph=graph_update, lr=hp["learning_rate"])
        self.curriculum = curriculum
        m, N, T = vec._mem, vec.num_envs, self.n_steps
        self.adv, self.ret = m.zeros((T, N)), m.zeros((T, N))
        self.num_timesteps, self.updates = 0, 0
        self.history = []
        self._gen = torch.Generator(device=self._torch_dev)
        self._gen.manual_seed(seed + 1)
        self._world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self._world = torch.distributed.get_world_size(group)
            for p in self.policy.parameters():   # identical initial weights on every rank
                torch.distributed.broadcast(p.data, src=0, group=group)
            self.actor.load_policy(self.policy)

    def _build_rollout(self):
        self.rollout = FusedRollout(self.vec, self.actor, self.n_steps, **self._rollout_kw)
        self._spec_at_capture = self.vec.spec_index
        if self.monitor is not None and self.rollout.warmup is not None:   # the env steps a capture takes outside the buffers
            self.monitor.fold(*self.rollout.warmup)

    def collect(self):
        """One rollout + advantages.  Returns the flattened training batch (views of the rollout buffers, no copies)."""
        buf = self.rollout.run()
        if self.monitor is not None:   # stream-ordered behind the rollout, before the update
            self.monitor.fold(buf["raw_rewards"], buf["dones"])
        gae(self.vec._lib, self.vec._mem, buf["rewards"], buf["values"], buf["dones"], self.rollout.last_value,
            self.hp["gamma"], self.hp["lam"], self.adv, self.ret)
        T, N = self.n_steps, self.vec.num_envs
        self.num_timesteps += T * N * self._world
        flat = lambda x, *s: torch.as_tensor(x).reshape((T * N,) + s)
        return {"obs": flat(buf["obs"], self.vec.obs_dim), "actions": flat(buf["actions"], 3), "values": flat(buf["values"]),
                "logp": flat(buf["logp"]), "adv": flat(self.adv), "returns": flat(self.ret)}

    def update(self, batch, lr=None, cliprange=None):
        """noptepochs x nminibatches steps on `batch` by the updater; a given `lr` stays in force.  Returns the steps' mean statistics."""
        hp = self.hp
        n, nmb = batch["obs"].shape[0], int(hp["nminibatches"])
        perms = (torch.randperm(n, device=self._torch_dev, generator=self._gen) for _ in range(int(hp["noptepochs"])))
        stats = self.learner.update(batch, perms, n // nmb, nmb, lr, hp["cliprange"] if cliprange is None else cliprange,
                                    hp["ent_coef"], hp["vf_coef"], hp["max_grad_norm"], world=self._world, group=self.group)
        self.updates += 1
        return stats

    def learn(self, total_timesteps, callback=None, log=None):
        from . import distributed as fd
        while self.num_timesteps < total_timesteps:
            batch = self.collect()
            stats = self.update(batch)
            summary = fd.gather_success(self.vec, self.group)    # episodes finished during this rollout, all ranks
            info = dict(stats, timesteps=self.num_timesteps, update=self.updates, episodes=summary["episodes"],
                        level=None if self.curriculum is None else self.curriculum.level)
            if summary["episodes"] > 0:
                info["success"] = dict(summary["success"])
                info["control_variation"] = summary["control_variation"]["all"]
            if self.monitor is not None:
                took = self.monitor.take(self.group)
                # (info["episodes"] stays gather_success's count, which "success" goes with; the monitor's own -- the episodes that
                # ended inside the folded buffers with a finite return -- is "monitor_episodes")
                info.update({("monitor_episodes" if k == "episodes" else k): v for k, v in took.items()})
                recent = self.monitor.window(100)
                info["ep_rew_mean_100"], info["ep_len_mean_100"] = recent["ep_rew_mean"], recent["ep_len_mean"]
                info["ep_info"] = summary if summary["episodes"] > 0 else _blank(summary)
            if self.curriculum is not None:
                info["level"] = self.curriculum.update(self.vec, summary)
                if self._rollout_kw["graph"] and self.vec.spec_index != self._spec_at_capture:
                    # (a captured rollout holds a kernel INSTANCE; the curriculum's ranges are read from memory and do not move it --
                    # a preset stays on its frozen kernel at every level, tests/test_shape_instance.py -- but a schedule whose
                    # update changes a folded value would: capture anew, fwg_replay_check refuses otherwise)
                    self._build_rollout()
            self.history.append(info)
            if log is not None:
                log(info)
            if callback is not None and callback(self, info) is False:
                break
        return self

    def deterministic_policy(self):
        """obs [N, ...] (raw, device tensor) -> mean action: VecNormalize with the statistics FROZEN at this moment (clip 10) in
        front of the policy network -- what `model.predict(obs, deterministic=True)` on a VecNormalize(training=False) env
        computes in the reference's evaluation (examples/evaluate_controller.py:93-100, :139)."""
        st = self.actor.get_stats()
        dev = self._torch_dev
        mean = torch.as_tensor(st["obs_mean"], dtype=torch.float32, device=dev)
        std = torch.sqrt(torch.as_tensor(st["obs_var"], dtype=torch.float32, device=dev) + 1e-8)
        pi = self.policy.pi

        @torch.no_grad()
        def act(obs):
            x = torch.as_tensor(obs, dtype=torch.float32, device=dev)
            return pi(((x.reshape(x.shape[0], -1) - mean) / std).clamp(-10.0, 10.0))
        return act

    def evaluate(self, scenarios, turbulence_intensity="none", first_step="raw", config=None):
        """The current policy on a test set, by the evaluation protocol on the device (evaluate.evaluate_on_set_device: what the
        reference's training script does at every fifth of a run, train_rl_controller.py --test-set-path) -> the table of
        evaluate.summarize().  One evaluation env (auto_reset off, the evaluation overrides on `config`, default: the training
        env's configuration) and one DeviceActor(training=False) are kept per scenario set; each call loads the current weights
        and the training head's statistics into that head and flies the set.  first_step: "raw" = the reference's protocol, the
        first action of every episode comes from the policy network on the UN-normalised reset observation
        (evaluate_controller.py:118); "normalised" = the head acts on every step.  Touches neither the training env nor the
        training head, and draws no random number."""
        import copy
        import hashlib
        import json
        from .actor import DeviceActor
        from .evaluate import DeviceEvaluation, evaluation_overrides
        from .vec_env import FixedWingVecEnv
        if first_step not in ("raw", "normalised"):
            raise ValueError("first_step must be 'raw' or 'normalised', not {!r}".format(first_step))
        key = hashlib.sha256(json.dumps([scenarios, turbulence_intensity, config if config is None or isinstance(config, (str, dict)) else str(config)],
                                        sort_keys=True).encode()).hexdigest()
        cache = self.__dict__.setdefault("_eval", {})
        if key not in cache:
            sim_kw = {"turbulence": turbulence_intensity != "none", "turbulence_intensity": turbulence_intensity}
            vec = FixedWingVecEnv(copy.deepcopy(self.vec.cfg) if config is None else config, num_envs=len(scenarios),
                                  config_kw=evaluation_overrides(False), sim_config_kw=sim_kw, auto_reset=False, seed=self.vec._seed,
                                  _backend=self.vec._mem)
            head = DeviceActor.for_env(vec, training=False, gamma=self.hp["gamma"], precise=self.actor.precise)
            cache[key] = (vec, head, DeviceEvaluation(vec, head, rewards=False))
        vec, head, run = cache[key]
        head.load_policy(self.policy)
        st = self.actor.get_stats()
        head.set_stats(st["obs_mean"], st["obs_var"], st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"])
        first = None
        if first_step == "raw":
            first = lambda obs: self.policy.pi(torch.as_tensor(obs).reshape(len(scenarios), -1))
        vec.seed(self.vec._seed)      # (the same turbulence realisation at every call: evaluations of one run are comparable)
        run.reset(scenarios, first)
        run.run()
        return run.result().table(vec.dt)

    def save(self, path):
        """Weights + VecNormalize statistics (the reference's save_model: model.pkl + save_running_average)."""
        st = self.actor.get_stats()
        sd = {k: v.detach().cpu().numpy() for k, v in self.policy.state_dict().items()}
        np.savez(path, **sd, **{"stat_" + k: np.asarray(v) for k, v in st.items()})

    def load(self, path):
        z = np.load(path)
        self.policy.load_state_dict({k: torch.as_tensor(z[k]) for k in z.files if not k.startswith("stat_")})
        self.actor.load_policy(self.policy)
        self.actor.set_stats(z["stat_obs_mean"], z["stat_obs_var"], float(z["stat_obs_count"]), float(z["stat_ret_mean"]),
                             float(z["stat_ret_var"]), float(z["stat_ret_count"]))
        return self
