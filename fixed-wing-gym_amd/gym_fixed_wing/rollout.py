"""On-device rollout collection for PPO-style training on FixedWingVecEnv (BASELINE.json
configs[4]).  Replaces the data path of the reference's training script -- `VecNormalize(SubprocVecEnv(...))` feeding
`PPO2(MlpPolicy)` (examples/train_rl_controller.py:223-231) -- with device-resident pieces: running observation /
return normalisation (VecNormalize), a 64-64 tanh MLP policy + value net (the architecture of the shipped
models/mlp_controller), and a rollout buffer filled without leaving the GPU.  The optimiser step is out of scope."""
import math

import numpy as np
import torch
from torch import nn


class RunningMeanStd(object):
    """Batched parallel-variance update (what stable-baselines' VecNormalize keeps as obs_rms / ret_rms)."""

    def __init__(self, shape, device=None, epsilon=1e-4):
        self.mean = torch.zeros(shape, dtype=torch.float32, device=device)
        self.var = torch.ones(shape, dtype=torch.float32, device=device)
        self.count = torch.full((), epsilon, dtype=torch.float32, device=device)   # a tensor: graph-capturable
        self._ones = None

    def update(self, x):
        # Batch moments through a ones-row GEMM on the deviations from the running mean, not Tensor.mean/var: torch's
        # multi-block dim-0 reductions return garbage from the second replay of a captured hipGraph on this stack
        # (ROCm 7.x / torch 2.10; found with tests/test_rollout.py, negative running variances), and the centred
        # form is also the numerically better one in fp32.
        x = x.reshape(-1, max(1, self.mean.numel()))
        b_count = x.shape[0]
        if self._ones is None or self._ones.shape[1] != b_count:
            self._ones = torch.ones((1, b_count), dtype=torch.float32, device=x.device)
        d = x - self.mean.reshape(1, -1)
        s1 = (self._ones @ d).reshape(self.mean.shape) / b_count
        s2 = (self._ones @ (d * d)).reshape(self.mean.shape) / b_count
        b_mean, b_var = self.mean + s1, (s2 - s1 * s1).clamp_min(0.0)
        delta = b_mean - self.mean
        tot = self.count + b_count
        m2 = self.var * self.count + b_var * b_count + delta * delta * (self.count * b_count / tot)
        self.mean.add_(delta * (b_count / tot))      # in place: the buffers keep their addresses under graph replay
        self.var.copy_(m2 / tot)
        self.count.copy_(tot)


class VecNormalizeDevice(object):
    def __init__(self, obs_shape, num_envs, device=None, clip_obs=10.0, clip_reward=10.0, gamma=0.99, training=True):
        self.obs_rms = RunningMeanStd(obs_shape, device)
        self.ret_rms = RunningMeanStd((), device)
        self.ret = torch.zeros(num_envs, dtype=torch.float32, device=device)
        self.clip_obs, self.clip_reward, self.gamma, self.training = clip_obs, clip_reward, gamma, training

    def obs(self, obs):
        if self.training:
            self.obs_rms.update(obs)
        return ((obs - self.obs_rms.mean) / torch.sqrt(self.obs_rms.var + 1e-8)).clamp(-self.clip_obs, self.clip_obs)

    def reward(self, rew, done):
        self.ret.mul_(self.gamma).add_(rew)
        if self.training:
            self.ret_rms.update(self.ret)
        out = (rew / torch.sqrt(self.ret_rms.var + 1e-8)).clamp(-self.clip_reward, self.clip_reward)
        self.ret.mul_(1.0 - done.to(self.ret.dtype))
        return out


class MlpPolicy(nn.Module):
    """Separate 64-64 tanh networks for the Gaussian policy mean and the value (stable-baselines MlpPolicy layout of
    the shipped MLP controller: pi_fc0/pi_fc1/pi, vf_fc0/vf_fc1/vf), state-independent log-std."""

    def __init__(self, obs_dim, act_dim=3, hidden=64):
        super().__init__()
        self.pi = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, act_dim))
        self.vf = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, 1))
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    @torch.no_grad()
    def act(self, obs, deterministic=False):
        mean = self.pi(obs)
        value = self.vf(obs).squeeze(-1)
        if deterministic:
            return mean, value, torch.zeros(obs.shape[0], device=obs.device)
        std = self.log_std.exp()
        noise = torch.randn_like(mean)
        action = mean + std * noise
        logp = (-0.5 * noise * noise - self.log_std - 0.5 * math.log(2 * math.pi)).sum(dim=-1)
        return action, value, logp


# The CNN controller's two unrecorded choices, settled against its published closed-loop rewards (tools/cnn_trace.py,
# profiles/cnn_architecture.txt): tanh after the conv, feature-major flatten (TF's NHWC reshape).  The HIP head has the same two
# as FWG_CNN_ACTIVATION / FWG_CNN_FEATURE_MAJOR (csrc/fwgym_actor.h).
CNN_ACTIVATION = "tanh"
CNN_FLATTEN = "nhwc"
_CNN_ACT = {"identity": lambda z: z, "tanh": torch.tanh, "relu": torch.relu}


class CnnFront(nn.Module):
    """The conv of the reference's CnnMlpPolicy (examples/train_rl_controller.py:179-197, --policy CNN): the (rows, features)
    observation through n_filters VALID kernels of rows x 1 (output height 1, shared by every feature), tanh, flattened
    feature-major -> rows-free vector of features * n_filters.  weight [rows][n_filters] (TF kernel [rows][1][1][n_filters])."""

    def __init__(self, obs_shape=(5, 12), n_filters=3):
        super().__init__()
        self.rows, self.features = int(obs_shape[0]), int(obs_shape[1])
        self.n_filters = int(n_filters)
        self.weight = nn.Parameter(torch.zeros(self.rows, self.n_filters))
        self.bias = nn.Parameter(torch.zeros(self.n_filters))

    @property
    def out_dim(self):
        return self.features * self.n_filters

    def forward(self, obs):
        x = obs.reshape(obs.shape[0], self.rows, self.features)
        y = _CNN_ACT[CNN_ACTIVATION](torch.einsum("brj,rc->bjc", x, self.weight) + self.bias)   # [B][features][filters]
        if CNN_FLATTEN != "nhwc":
            y = y.transpose(1, 2)
        return y.reshape(obs.shape[0], -1)                                                    # k = j * n_filters + c


class CnnMlpPolicy(nn.Module):
    """The CNN controller's policy (examples/models/cnn_controller): one conv shared by pi and vf (CnnFront), then the
    MlpPolicy's separate 64-64 tanh networks on its 36 outputs.  Same contract as MlpPolicy: `pi(obs)` -> mean, `vf(obs)` ->
    value, `log_std`; obs [N, rows * features] or [N, rows, features]."""

    def __init__(self, obs_shape=(5, 12), n_filters=3, act_dim=3, hidden=64):
        super().__init__()
        self.obs_shape = (int(obs_shape[0]), int(obs_shape[1]))
        self.conv = CnnFront(obs_shape, n_filters)
        k = self.conv.out_dim
        self.pi = nn.Sequential(self.conv, nn.Linear(k, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, act_dim))
        self.vf = nn.Sequential(self.conv, nn.Linear(k, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, 1))
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    act = MlpPolicy.act


def collect_rollout(vec, policy, norm, n_steps, obs=None):
    """n_steps of policy inference + env step for all envs, everything on the device.  Returns the rollout buffer
    {obs, actions, values, logp, rewards, dones} ([n_steps, N, ...]) and the last normalised observation."""
    N = vec.num_envs
    raw = vec._obs.reshape(N, -1) if obs is None else obs
    raw = torch.as_tensor(raw)
    dev = raw.device
    buf = {"obs": torch.empty((n_steps, N, raw.shape[1]), device=dev), "actions": torch.empty((n_steps, N, 3), device=dev),
           "values": torch.empty((n_steps, N), device=dev), "logp": torch.empty((n_steps, N), device=dev),
           "rewards": torch.empty((n_steps, N), device=dev), "dones": torch.empty((n_steps, N), dtype=torch.uint8, device=dev)}
    cur = norm.obs(raw)
    for t in range(n_steps):
        action, value, logp = policy.act(cur)
        buf["obs"][t], buf["actions"][t], buf["values"][t], buf["logp"][t] = cur, action, value, logp
        if hasattr(vec, "step_device") and isinstance(vec._obs, torch.Tensor):
            o, r, d = vec.step_device(action.contiguous())
        else:
            o, r, d, _ = vec.step(action.cpu().numpy())
            o, r, d = torch.as_tensor(o).reshape(N, -1), torch.as_tensor(r), torch.as_tensor(d)
        buf["rewards"][t] = norm.reward(torch.as_tensor(r).to(dev), torch.as_tensor(d).to(dev))
        buf["dones"][t] = torch.as_tensor(d).to(dev)
        cur = norm.obs(torch.as_tensor(o).reshape(N, -1).to(dev))
    return buf, cur


class GraphedRollout(object):
    """The whole n-step rollout (policy forward, normalisation, fused env step, buffer writes) captured ONCE into a
    hipGraph (torch.cuda.CUDAGraph) and replayed: no per-kernel host launch cost.  Needs the env's graph mode (the
    global step counter lives on the device, see include/fwgym.h) and an even n_steps."""

    def __init__(self, vec, policy, norm, n_steps):
        assert n_steps % 2 == 0, "graph mode double-buffers the step counter: capture an even number of steps"
        self.vec, self.policy, self.norm, self.n_steps = vec, policy, norm, n_steps
        N, D = vec.num_envs, vec.obs_dim
        dev = vec._obs.device
        self.buf = {"obs": torch.empty((n_steps, N, D), device=dev), "actions": torch.empty((n_steps, N, 3), device=dev),
                    "values": torch.empty((n_steps, N), device=dev), "logp": torch.empty((n_steps, N), device=dev),
                    "rewards": torch.empty((n_steps, N), device=dev),
                    "dones": torch.empty((n_steps, N), dtype=torch.uint8, device=dev)}
        self.action = torch.zeros((N, 3), device=dev)
        # row-log envs: zero-copy windows only when the chunk is a whole number of window periods (they stay right under replay
        # then); any other length gets the gathered copy per step
        period = getattr(vec, "obs_window_period", 0)
        vec.set_graph_mode(True, obs="view" if (period and n_steps % period == 0) else "gather")
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):          # warm-up outside capture (allocations, lazy initialisation)
            self._body(2)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        self._parity = vec.capture_begin(n_steps)
        with torch.cuda.graph(self.graph):
            self._body(n_steps)
        vec.capture_end()

    def _body(self, n):
        vec, buf = self.vec, self.buf
        N = vec.num_envs
        cur = self.norm.obs(vec._obs.reshape(N, -1))
        for t in range(n):
            action, value, logp = self.policy.act(cur)
            self.action.copy_(action)
            buf["obs"][t].copy_(cur); buf["actions"][t].copy_(action); buf["values"][t].copy_(value); buf["logp"][t].copy_(logp)
            o, r, d = vec.step_device(self.action)
            buf["rewards"][t].copy_(self.norm.reward(r, d))
            buf["dones"][t].copy_(d)
            cur = self.norm.obs(o.reshape(N, -1))

    def run(self):
        self.vec.replay_check(self._parity)
        self.graph.replay()
        self.vec.note_replayed_steps(self.n_steps)
        return self.buf


# ----------------------------------------------------------------------------------------------------------------------
# The same rollout on the HIP rollout head (gym_fixed_wing.actor.DeviceActor): three launches per step
# ----------------------------------------------------------------------------------------------------------------------
class FusedRollout(object):
    """n-step rollouts of FixedWingVecEnv under a DeviceActor, filling {obs, actions, values, logp, rewards, dones}
    ([n_steps, N, ...], normalised observations/rewards as VecNormalize + PPO2 store them) plus `last_value` (the
    bootstrap value of the observation after the last step).  Per step: fwg_step (which also leaves the batch moments for
    the attached head) and fwg_actor_act --
    the act that follows step t writes the rollout slice t+1 directly, so nothing is copied except the carried-over
    slice 0.  `graph=True` captures the whole rollout into one hipGraph (n_steps must be even).

    `fused` (opt-in: fused=True, fused="auto" = wherever fwg_rollout_available, or FWGYM_ROLLOUT_FUSED=1): act t and env step t run as ONE launch (fwg_rollout_step) -- a rollout is
    then [env step 0] [act + step] x (n - 1) [act n]: n + 1 launches instead of 2 n, bit-identical buffers.  `tap(t, obs, rew,
    done)` (eager mode only) is called after every env step with the env's raw output tensors (tests, logging).

    `raw_rewards=True`: the rollout also owns buf["raw_rewards"] (float32 [n_steps, N]) and env step t writes its reward into
    row t INSTEAD of vec._rew (fwg_step's reward_out argument: the same bytes to another address, no extra launch, no copy); the
    head and an attached FlightRecorder read that row.  It is what gym_fixed_wing.monitor.EpisodeMonitor folds.  The one-launch
    step reads the previous reward and writes the new one through ONE pointer (reward_io), so it cannot do this: fused=True is
    refused and None / "auto" take the two-launch path.

    `goals=log` (a gym_fixed_wing.goal.GoalLog of this env and n_steps): one fwg_goal_observe launch writes the goal rows of the
    log, row 0 at the start of every rollout body (right whatever came before: a reset, the capture's warm-up steps, the previous
    rollout) and row t + 1 behind env step t, eagerly and under graph=True.  Needs raw_rewards=True (log.relabel reads them) and
    the two-launch path, with the refusals of raw_rewards."""

    def __init__(self, vec, actor, n_steps, graph=False, fused=None, tap=None, raw_rewards=False, goals=None):
        self.vec, self.actor, self.n_steps = vec, actor, int(n_steps)
        m, N, D, A = vec._mem, vec.num_envs, vec.obs_dim, actor.act_dim
        self.buf = {"obs": m.zeros((n_steps, N, D)), "actions": m.zeros((n_steps, N, A)), "values": m.zeros((n_steps, N)),
                    "logp": m.zeros((n_steps, N)), "rewards": m.zeros((n_steps, N)), "dones": m.zeros((n_steps, N), "u8")}
        self.raw_rewards = bool(raw_rewards)
        self.goals = goals
        if goals is not None:
            if not self.raw_rewards:
                raise ValueError("FusedRollout(goals=log): relabelling reads the raw reward of every step -- pass raw_rewards=True")
            if goals.vec is not vec or goals.n_steps != self.n_steps:
                raise ValueError("FusedRollout(goals=log): the GoalLog belongs to another env or another rollout length")
        self.warmup = None   # graph=True with raw_rewards: (raw_rewards [2, N], dones [2, N]) of the capture's two warm-up steps
        if self.raw_rewards:
            self.buf["raw_rewards"] = m.zeros((n_steps, N))
        # the head's outputs for the CURRENT observation, carried from one rollout to the next
        self.cur = {"obs": m.zeros((N, D)), "actions": m.zeros((N, A)), "values": m.zeros((N,)), "logp": m.zeros((N,))}
        self.last_value = self.cur["values"]
        self._primed = False
        self._graph = None
        # the env step kernel leaves the batch moments itself (two launches per step) -- except with row-log observations,
        # where the lagged rows never pass through the step kernel: then the head reads the window out of the log in place
        # (fwg_actor_set_obs_log: position read on the device, replay-safe) and takes the moments in a launch of its own
        self._attached = not getattr(vec, "obs_log_rows", 0)
        if self._attached:
            actor.attach(vec)
        else:
            actor.set_obs_log(vec)
        can_fuse = self._attached and hasattr(actor, "rollout_available") and actor.rollout_available(vec)
        # a FlightRecorder (gym_fixed_wing.recorder) records behind every fwg_step launch: the one-launch step has no such
        # boundary, so "auto" / None take the two-launch path with a recorder attached and fused=True is refused
        recording = getattr(vec, "_recorder", None) is not None
        if self.raw_rewards and fused and fused != "auto":
            raise ValueError("FusedRollout(fused=True, raw_rewards=True): the one-launch step (fwg_rollout_step) keeps the reward in "
                             "one in-out buffer and cannot write rollout rows -- use the two-launch path (fused=False, None or 'auto')")
        recording = recording or self.raw_rewards   # (either way: the two-launch path)
        if fused == "auto":   # the one-launch step wherever it is available
            fused = bool(can_fuse) and not recording
        if fused and recording:
            raise ValueError("FusedRollout(fused=True): a FlightRecorder is attached to this env and the one-launch step "
                             "(fwg_rollout_step) cannot be recorded -- use the two-launch path (fused=False, None or 'auto')")
        if fused and not can_fuse:
            raise ValueError("FusedRollout(fused=True): fwg_rollout_step is not available for this env / head (needs a specialised "
                             "kernel, the dense observation batch and an attached head)")
        # OPT-IN (fused=True, or FWGYM_ROLLOUT_FUSED=1 for fused=None): tests/test_rollout.py::test_fused_launch_equals_two_launches_on_gpu
        # failed twice in ~25 runs of the whole GPU suite in round 4 and the cause was never found (2 000+ clean iterations since,
        # in isolation and in suite context: profiles/r05_soak.txt) -- until it is, the path whose every launch boundary is a
        # kernel boundary stays the default and the one-launch step is something a caller asks for (bench.py does, and says so)
        import os
        self.fused = (can_fuse and not recording and os.environ.get("FWGYM_ROLLOUT_FUSED", "0") == "1") if fused is None else bool(fused)
        self.tap = tap
        if graph:
            self._capture()

    def _prime(self):
        if not self._primed:   # first observation after reset(): no transition led here
            c = self.cur
            o = self.vec._obs if self._attached else self.vec._obs_buf
            self.actor.observe(o)
            self.actor.act(o, norm_obs=c["obs"], action=c["actions"], value=c["values"], logp=c["logp"])
            self._primed = True

    def _step(self, action, nxt, reward_out=None, done_out=None, raw_out=None):
        """One env step under `action`, then the head on the new observation writing into the slices of `nxt`.  raw_out: where
        the env step writes its rewards (default: the env's own buffer)."""
        vec, actor = self.vec, self.actor
        # (without raw_out the call is the one it always was)
        o, r, d = vec.step_device(action, want_obs=self._attached, **({} if raw_out is None else {"reward_out": raw_out}))
        if not self._attached:
            o = vec._obs_buf    # the row log itself: the head windows it on the device
            actor.observe(o, r, d)
        actor.act(o, reward=r, done=d, norm_obs=nxt["obs"], action=nxt["actions"], value=nxt["values"], logp=nxt["logp"],
                  norm_reward=reward_out, done_out=done_out)

    def _body(self):
        buf, cur, n = self.buf, self.cur, self.n_steps
        vec, actor = self.vec, self.actor
        tap = self.tap if self._graph is None and not getattr(self, "_capturing", False) else None
        for k in ("obs", "actions", "values", "logp"):
            buf[k][0][...] = cur[k]
        if self.fused:
            # env step 0 under the carried-over actions; then [act t + env step t] in one launch each; then act n
            o, r, d = vec.step_device(buf["actions"][0])
            if tap is not None:
                tap(0, o, r, d)
            for t in range(1, n):
                o, r, d = actor.rollout_step(vec, norm_obs=buf["obs"][t], action=buf["actions"][t], value=buf["values"][t],
                                             logp=buf["logp"][t], norm_reward=buf["rewards"][t - 1], done_out=buf["dones"][t - 1])
                if tap is not None:
                    tap(t, o, r, d)
            actor.act(o, reward=r, done=d, norm_obs=cur["obs"], action=cur["actions"], value=cur["values"], logp=cur["logp"],
                      norm_reward=buf["rewards"][n - 1], done_out=buf["dones"][n - 1])
            return
        goals = self.goals
        if goals is not None:
            goals.observe(0)
        for t in range(n):
            nxt = cur if t == n - 1 else {k: buf[k][t + 1] for k in cur}
            raw = buf["raw_rewards"][t] if self.raw_rewards else None
            self._step(buf["actions"][t], nxt, buf["rewards"][t], buf["dones"][t], raw)
            if goals is not None:
                goals.observe(t + 1)
            if tap is not None:
                tap(t, self.vec._obs, self.vec._rew if raw is None else raw, self.vec._done)

    def _capture(self):
        import torch
        assert self.n_steps % 2 == 0, "graph mode double-buffers step counter and statistics: capture an even number of steps"
        vec = self.vec
        dev = vec._obs.device
        vec.set_graph_mode(True)
        self._prime()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # warm-up outside capture: two env steps, every kernel of the body launched once
            if self.fused:
                c = self.cur
                vec.step_device(c["actions"])
                o, r, d = self.actor.rollout_step(vec, norm_obs=c["obs"], action=c["actions"], value=c["values"], logp=c["logp"])
                self.actor.act(o, reward=r, done=d, norm_obs=c["obs"], action=c["actions"], value=c["values"], logp=c["logp"])
            else:
                # (the two warm-up steps are env steps like any other: with raw_rewards their rewards and done flags are kept in
                # `warmup`, for the caller to fold before the first rollout -- otherwise every env's open episode would lose them)
                warm = self.warmup = (vec._mem.zeros((2, vec.num_envs)), vec._mem.zeros((2, vec.num_envs), "u8")) if self.raw_rewards else None
                for i in range(2):
                    self._step(self.cur["actions"], self.cur, None, warm[1][i] if warm else None, warm[0][i] if warm else None)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        self._parity = vec.capture_begin(self.n_steps)
        self._capturing = True
        with torch.cuda.graph(graph):
            self._body()
        self._capturing = False
        vec.capture_end()
        self._graph = graph

    def run(self):
        self._prime()
        if self._graph is not None:
            self.vec.replay_check(self._parity)
            self._graph.replay()
            self.vec.note_replayed_steps(self.n_steps)
        else:
            self._body()
        return self.buf
