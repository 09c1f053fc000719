"""Scenario-replay evaluation on the vectorised env -- the protocol of the reference's
examples/evaluate_controller.py:44-169 (evaluate_model_on_set), with every scenario of the test set running in its own
env slot at the same time instead of being queued onto a handful of sub-process envs.

A scenario is {"state": {21 floats}, "target": {roll, pitch, Va}} (the record format of get_initial_state,
fixed_wing.py:848-862).  Overrides applied exactly as the reference does (:68-78): steps_max 1500, on_success "done",
streak 100 @ fraction 1, bounds 5deg/5deg/2 m/s, PID => scale_space False, turbulence via sim_config_kw.
Returns the reference's result layout: {metric: {state: [per scenario]}, "rewards": [per scenario [per step]]}, all in
SCENARIO order (the reference stores the metric lists in completion order, evaluate_controller.py:127-137)."""
import copy
import ctypes
import math

import numpy as np

from .pid import BatchedPID
from .vec_env import FixedWingVecEnv

METRICS = ("success", "control_variation", "rise_time", "overshoot", "settling_time")


def evaluation_overrides(use_pid, config_kw=None):
    kw = {} if config_kw is None else copy.deepcopy(config_kw)
    kw.update({"steps_max": 1500, "target": {"on_success": "done", "success_streak_fraction": 1,
                                             "success_streak_req": 100,
                                             "states": {0: {"bound": 5}, 1: {"bound": 5}, 2: {"bound": 2}}}})
    if use_pid:
        kw["action"] = {"scale_space": False}
    return kw


def evaluate_on_set(scenarios, config_path=None, policy=None, config_kw=None, turbulence_intensity="none", device=0,
                    seed=0, metrics=METRICS, pid_gains=None, first_step_policy=None, **vec_kw):
    """policy: None => the PID baseline; otherwise a callable obs[N, ...] (device tensor) -> actions[N, 3].

    first_step_policy: the callable that produces the FIRST action of every episode (default: `policy`).  The reference's
    evaluation wraps the envs in VecNormalize but takes the observation of a scenario's reset straight from
    env_method("reset", ...) (evaluate_controller.py:118), which bypasses the wrapper: the model's first action of every
    episode is computed from the UN-normalised observation, all later ones from normalised ones (:139, :153).  The published
    RL results carry that step (second-step reward error against eval_res_RL_MLP_none.npy 0.023 -> 0.0006 with it, control
    variation 0.29 -> 0.36 against the published 0.41); pass the policy WITHOUT its observation normalisation here to fly the
    reference's protocol to the letter."""
    import torch
    use_pid = policy is None
    n = len(scenarios)
    kw = evaluation_overrides(use_pid, config_kw)
    sim_kw = {"turbulence": turbulence_intensity != "none", "turbulence_intensity": turbulence_intensity}
    vec = FixedWingVecEnv(config_path, num_envs=n, device=device, config_kw=kw, sim_config_kw=sim_kw, auto_reset=False,
                          seed=seed, **vec_kw)
    names = vec.target_names
    states = {k: np.array([s["state"][k] for s in scenarios], dtype=np.float32) for k in scenarios[0]["state"]}
    targets = {k: np.array([s["target"][k] for s in scenarios], dtype=np.float32) for k in names}
    obs = vec.reset(states=states, targets=targets)
    as_t = (lambda x: x) if isinstance(obs, torch.Tensor) else (lambda x: torch.as_tensor(np.asarray(x)))
    obs = as_t(obs)
    dev = obs.device
    if use_pid:
        obs_names = [v["name"] for v in vec.cfg["observation"]["states"]]
        try:
            i_phi, i_theta, i_va = obs_names.index("roll"), obs_names.index("pitch"), obs_names.index("Va")
            i_om = [obs_names.index("omega_p"), obs_names.index("omega_q"), obs_names.index("omega_r")]
        except ValueError:
            raise ValueError("When using PID roll, pitch, Va, omega_p, omega_q, omega_r must be part of the "
                             "observation vector.")
        pid = BatchedPID(n, dt=vec.dt, device=dev)
        for k, v in (pid_gains or {}).items():
            setattr(pid, k, v)
        pid.set_reference(*(torch.as_tensor(targets[k], device=dev) for k in names))
    active = torch.ones(n, dtype=torch.bool, device=dev)
    rewards = [[] for _ in range(n)]
    res = {m: {} for m in metrics}
    finished = {}
    for t_step in range(vec.cfg["steps_max"] + 1):
        if use_pid:
            row = obs.reshape(n, -1)
            act = pid.get_action(row[:, i_phi], row[:, i_theta], row[:, i_va], row[:, i_om])
        else:
            act = as_t((first_step_policy if (t_step == 0 and first_step_policy is not None) else policy)(obs)).to(dev)
        act = torch.where(active[:, None], act.float(), torch.zeros_like(act, dtype=torch.float32))
        obs, rew, done, infos = vec.step(act if isinstance(vec._obs, torch.Tensor) else act.cpu().numpy())
        obs, rew, done = as_t(obs), as_t(rew), as_t(done).bool()
        if use_pid:  # the reference refreshes the PID reference from info["target"] (evaluate_controller.py:146-149)
            tg = as_t(vec._target)
            pid.set_reference(tg[:, names.index("roll")], tg[:, names.index("pitch")], tg[:, names.index("Va")])
        r_host, a_host = rew.cpu().numpy(), active.cpu().numpy()
        for i in np.nonzero(a_host)[0]:
            rewards[i].append(float(r_host[i]))
        newly = (done.to(dev) & active).cpu().numpy()
        for i in np.nonzero(newly)[0]:
            finished[int(i)] = dict(infos[int(i)])
        active = active & ~done.to(dev)
        if not bool(active.any()):
            break
    for m in metrics:
        for i in range(n):
            val = finished[i][m] if i in finished else {}
            for state, v in val.items():
                res[m].setdefault(state, [None] * n)[i] = v
    res["rewards"] = rewards
    res["termination"] = [finished[i].get("termination") if i in finished else None for i in range(n)]
    vec.close()
    return res


def summarize(res, dt=0.01):
    """The numbers of the reference's results table (examples/README.md:33-47; print_results,
    evaluate_controller.py:32-41): success rates in %, times in seconds, overshoot in %, metrics other than success
    averaged over the successful episodes."""
    ok = np.array([bool(v) for v in res["success"]["all"]])
    out = {"success_%": {k: 100.0 * np.mean([bool(x) for x in v]) for k, v in res["success"].items()}}
    for m, scale in (("rise_time", dt), ("settling_time", dt), ("overshoot", 100.0), ("control_variation", 1.0)):
        if m in res:
            out[m] = {k: float(np.nanmean([x * scale if (o and x is not None) else np.nan
                                           for x, o in zip(v, ok)])) for k, v in res[m].items()}
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The same protocol with the loop on the device (include/fwgym.h "Evaluation").  evaluate_on_set above stays the yardstick.
# ----------------------------------------------------------------------------------------------------------------------
class EvalResult(object):
    """Per-scenario results of a device evaluation as host arrays, scenario order: length [N] (steps of the first episode),
    termination [N] (FWG_TERM_* of its end, 0 = still running at the step limit of the loop), metrics [N_METRICS][N] (the metrics
    block's column at that end, NaN while running), rewards [T][N] (NaN after an episode's end) or None."""

    def __init__(self, length, termination, metrics, rewards, metrics_dict, target_names, has_bound, metric_names):
        self.length, self.termination, self.metrics, self.rewards = length, termination, metrics, rewards
        self._metrics_dict, self._names, self._has_bound, self._metric_names = metrics_dict, target_names, has_bound, metric_names

    def as_reference_layout(self, metrics=METRICS):
        """Exactly the dict evaluate_on_set returns."""
        from . import _native as nat
        n = len(self.length)
        finished = {i: dict(self._metrics_dict(self.metrics[:, i]), termination=nat.term_name(self.termination[i]))
                    for i in range(n) if self.termination[i] != 0}
        res = {m: {} for m in metrics}
        for m in metrics:
            for i in range(n):
                val = finished[i][m] if i in finished else {}
                for state, v in val.items():
                    res[m].setdefault(state, [None] * n)[i] = v
        if self.rewards is None:
            res["rewards"] = None
        else:
            res["rewards"] = [[float(r) for r in self.rewards[:self.length[i], i]] for i in range(n)]
        res["termination"] = [finished[i].get("termination") if i in finished else None for i in range(n)]
        return res

    def _rows(self, metric):
        """{state: row of the metrics block} of one metric, the states metrics_dict lists for it."""
        from . import _native as nat
        names = list(self._names)
        bounded = [(s, k) for k, s in enumerate(names) if self._has_bound[k]] + [("all", 3)]
        if metric not in self._metric_names:
            return {}
        if metric == "success":
            return {s: nat.M_SUCCESS + k for s, k in bounded}
        if metric == "settling_time":
            return {s: nat.M_SETTLING_TIME + k for s, k in bounded}
        if metric == "control_variation":
            return {"all": nat.M_CONTROL_VARIATION}
        base = {"rise_time": nat.M_RISE_TIME, "overshoot": nat.M_OVERSHOOT}[metric]
        return {s: base + k for k, s in enumerate(names)}

    def table(self, dt=0.01):
        """The numbers of summarize(), computed on the arrays (no per-scenario Python objects)."""
        done = self.termination != 0
        succ = {s: done & (self.metrics[r] == 1.0) for s, r in self._rows("success").items()}
        ok = succ["all"]
        out = {"success_%": {s: 100.0 * np.mean(v) for s, v in succ.items()}}
        for m, scale in (("rise_time", dt), ("settling_time", dt), ("overshoot", 100.0), ("control_variation", 1.0)):
            out[m] = {s: float(np.nanmean(np.where(ok, self.metrics[r].astype(np.float64) * scale, np.nan)))
                      for s, r in self._rows(m).items()}
        return out


class DeviceEvaluation(object):
    """The loop of evaluate_on_set_device on an env built for it (auto_reset=False, num_envs == number of scenarios):
    reset(scenarios) -> run(chunk) -> result().  Per step: controller -> fwg_finish_episodes -> fwg_eval_advance -> fwg_step, all
    stream-ordered launches on buffers owned here; the host reads one flag per chunk.  controller: a DevicePID or a
    DeviceActor(training=False)."""

    def __init__(self, vec, controller, rewards=True):
        from . import _native as nat
        from .pid import DevicePID
        if vec.auto_reset:
            raise ValueError("the evaluation protocol needs FixedWingVecEnv(auto_reset=False)")
        self.vec, self.controller, self._nat = vec, controller, nat
        self.is_pid = isinstance(controller, DevicePID)
        m, N = vec._mem, vec.num_envs
        if not self.is_pid:
            if controller.num_envs != N or controller.obs_dim != vec.obs_dim:
                raise ValueError("the head serves {} envs x {} observations, the evaluation env has {} x {}".format(
                    controller.num_envs, controller.obs_dim, N, vec.obs_dim))
            if controller.training:
                raise ValueError("the evaluation protocol needs a head with frozen statistics: DeviceActor(training=False)")
            self._head_out = (m.zeros((N, vec.obs_dim)), m.zeros((N,)), m.zeros((N,)))   # norm_obs, value, logp: unused outputs
        self.max_steps = int(vec.cfg["steps_max"]) + 1   # (evaluate_on_set: range(steps_max + 1))
        self.actions = m.zeros((N, 3))
        self.active, self.length, self.termination = m.zeros((N,), "u8"), m.zeros((N,), "i32"), m.zeros((N,), "u8")
        self.metrics_final = m.zeros((nat.N_METRICS, N))
        self.trace = m.zeros((self.max_steps, N)) if rewards else None
        self.t, self._finalised = 0, True

    def reset(self, scenarios, first_step_policy=None):
        vec, m = self.vec, self.vec._mem
        n, names = len(scenarios), vec.target_names
        if n != vec.num_envs:
            raise ValueError("{} scenarios for an env of {}".format(n, vec.num_envs))
        states = {k: np.array([s["state"][k] for s in scenarios], dtype=np.float32) for k in scenarios[0]["state"]}
        targets = {k: np.array([s["target"][k] for s in scenarios], dtype=np.float32) for k in names}
        obs = vec.reset(states=states, targets=targets)
        self.active[...] = 1
        self.length[...] = 0
        self.termination[...] = 0
        self.metrics_final[...] = math.nan
        if self.is_pid:
            self.controller.reset()
            # fwg_reset writes no info["target"]: the PID's first reference is the scenario's target (evaluate_controller.py:120-124)
            vec._target[...] = m.from_host(np.stack([targets[k] for k in names], axis=1))
        self._first = None
        if first_step_policy is not None and not self.is_pid:
            import torch
            with torch.no_grad():
                self._first = torch.as_tensor(first_step_policy(obs)).to(self.actions.device).float().reshape(n, 3).contiguous()
        self.t, self._finalised = 0, False

    def _advance(self, actions):
        vec, m, nat = self.vec, self.vec._mem, self._nat
        null = ctypes.c_void_p()
        nat.check(vec._lib, vec._lib.fwg_eval_advance(
            vec.num_envs, self.t, m.ptr(vec._rew), m.ptr(vec._done), m.ptr(vec._term), m.ptr(vec._metrics), m.ptr(self.active),
            m.ptr(self.length), m.ptr(self.termination), m.ptr(self.metrics_final), m.ptr(self.trace) if self.trace is not None else null,
            self.max_steps, m.ptr(actions) if actions is not None else null, m.stream()))

    def _step(self):
        vec = self.vec
        if self.t == 0 and self._first is not None:
            self.actions[...] = self._first
        elif self.is_pid:
            self.controller.act(self.actions)
        else:
            # (a row-log env: the dense copy of the current window, gathered on the device -- the values of the log)
            self.controller.act(vec.obs_dense() if vec.obs_log_rows else vec._obs, norm_obs=self._head_out[0], action=self.actions,
                                value=self._head_out[1], logp=self._head_out[2], deterministic=True)
        vec.finish_episodes()
        self._advance(self.actions)
        vec.step_device(self.actions, want_obs=self.is_pid, target_out=True)
        self.t += 1

    def run(self, chunk=100):
        """Flies until every scenario's first episode has ended (looked at once per `chunk` steps) or the step limit."""
        if self._finalised:
            raise RuntimeError("reset() first")
        chunk = max(1, int(chunk))
        while self.t < self.max_steps:
            for _ in range(min(chunk, self.max_steps - self.t)):
                self._step()
            if not self.vec._mem.to_host(self.active).any():
                break
        self.vec.finish_episodes()
        self._advance(None)    # folds the last step
        self._finalised = True
        return self.t

    def result(self):
        vec, m = self.vec, self.vec._mem
        rewards = None if self.trace is None else np.array(m.to_host(self.trace[:self.t]))
        has_bound = [t.get("bound", None) is not None for t in vec.cfg["target"]["states"]]
        return EvalResult(np.array(m.to_host(self.length)), np.array(m.to_host(self.termination)), np.array(m.to_host(self.metrics_final)),
                          rewards, vec.metrics_dict, list(vec.target_names), has_bound, [x["name"] for x in vec.cfg.get("metrics", [])])


def evaluate_on_set_device(scenarios, config_path=None, controller=None, config_kw=None, turbulence_intensity="none", device=0,
                           seed=0, first_step_policy=None, chunk=100, rewards=True, **vec_kw):
    """evaluate_on_set with the loop on the device: no host read inside a chunk of `chunk` steps, one ("any scenario still
    flying?") after each.  controller: None = the PID baseline (DevicePID; a dict = its gains), otherwise a
    DeviceActor(training=False) for len(scenarios) envs, MLP or CNN.  first_step_policy: as in evaluate_on_set, evaluated once,
    eagerly, for the first action.  Launches are eager (no graph: its warm-up steps would have to fly the evaluated episodes,
    and the tracker's step count travels by value).  Returns an EvalResult."""
    from .pid import DevicePID
    use_pid = controller is None or isinstance(controller, dict)
    kw = evaluation_overrides(use_pid, config_kw)
    sim_kw = {"turbulence": turbulence_intensity != "none", "turbulence_intensity": turbulence_intensity}
    vec = FixedWingVecEnv(config_path, num_envs=len(scenarios), device=device, config_kw=kw, sim_config_kw=sim_kw, auto_reset=False,
                          seed=seed, **vec_kw)
    try:
        run = DeviceEvaluation(vec, DevicePID(vec, controller) if use_pid else controller, rewards=rewards)
        run.reset(scenarios, first_step_policy)
        run.run(chunk)
        return run.result()
    finally:
        vec.close()
