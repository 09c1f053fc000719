"""GoalSpec / GoalVecEnv / GoalLog -- the reference's FixedWingAircraftGoal (a gym.GoalEnv for hindsight experience replay,
fixed_wing.py:1165-1277) for a whole FixedWingVecEnv, on the device.

The single-env class (gym_fixed_wing.fixed_wing.FixedWingAircraftGoal) builds its goal views with host reads of one env and
evaluates compute_reward one transition at a time in Python float64.  A hindsight buffer relabels every transition it stores: one
rollout of 65 536 envs x 128 steps is 8.4 M compute_reward calls.  Here the goal views come from one small launch behind each
reset / step (fwg_goal_observe), compute_reward is one launch per batch (fwg_goal_reward) and HER's "future" strategy over a
rollout is one launch (fwg_goal_relabel); csrc/fwgym_goal.h, include/fwgym.h "Goal env".

    GoalSpec.from_env(vec)   which target states are goals and their scaling, from cfg["observation"]["goals"]; refuses what the
                             reward of a substituted goal cannot be defined for, with the names of the configuration
    GoalVecEnv(vec)          the dict API in batch: reset / step / step_device return {"observation", "achieved_goal",
                             "desired_goal"}, get_goal_limits(), compute_reward(achieved_goal, desired_goal, info) on batches
    GoalLog(vec, n_steps)    the goal rows of a FusedRollout(..., goals=log) and relabel() of its buffers

Nothing of the env changes while none of them is attached: they launch behind the env's own calls, over buffers of their own."""
import ctypes

import numpy as np

from . import _native as nat
from .spaces import Box, DictSpace

GOAL_STATES = ("roll", "pitch", "Va")   # the words the kernels can serve for the committed state (csrc/fwgym_record.h rec_derived)


class GoalSpec(object):
    """names / k / mean / var of the goals; struct(mode) is the fwg_goal_spec the C calls take."""

    def __init__(self, names, k, mean, var):
        self.names, self.k = list(names), [int(i) for i in k]
        self.mean, self.var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
        self.n = len(self.names)

    @classmethod
    def from_env(cls, vec, reward=True, relabel=False):
        """reward: also check that the reward of a substituted goal is defined (compute_reward, relabel); relabel: and that the goal is
        constant within an episode.  The C calls refuse the same configurations by factor index; here they are named."""
        cfg = vec.cfg
        goals = cfg["observation"].get("goals", None)
        if not goals:
            raise ValueError("the configuration has no observation.goals: nothing to condition on")
        if len(goals) > 3:
            raise ValueError("at most 3 goals, observation.goals lists {}".format(len(goals)))
        targets = list(vec.target_names)
        names = [g["name"] for g in goals]
        for name in names:
            if name not in targets:
                raise ValueError("goal '{}' is not one of the target states {}".format(name, targets))
            if name not in GOAL_STATES:
                raise ValueError("goal '{}': a goal must be one of {}".format(name, list(GOAL_STATES)))
            if names.count(name) > 1:
                raise ValueError("goal '{}' is listed twice".format(name))
        for g in goals:
            if not g.get("var", 1.0):
                raise ValueError("goal '{}' has var 0".format(g["name"]))
        if reward:
            cls.check_reward(cfg, names)
        if relabel:
            cls.check_relabel(cfg)
        return cls(names, [targets.index(n) for n in names], [g.get("mean", 0.0) for g in goals], [g.get("var", 1.0) for g in goals])

    @staticmethod
    def check_reward(cfg, names):
        rcfg = cfg["reward"]
        if rcfg.get("randomize_scaling", False):
            raise ValueError("reward.randomize_scaling draws the factor scalings per env and episode: the reward of a substituted goal "
                             "is not defined by the transition alone")
        bounded = [t["name"] for t in cfg["target"]["states"] if t.get("bound", None) is not None]
        for f in rcfg["factors"]:
            label = "reward factor '{}' ({} / {})".format(f.get("name"), f["class"], f.get("type"))
            if f["class"] == "state":
                if f.get("type") == "int_error":
                    raise ValueError(label + " sums the errors of earlier steps, which a transition does not carry")
                if f["name"] not in names:
                    raise ValueError(label + " reads '{}', which is not a goal {}".format(f["name"], names))
            if f["class"] == "goal":
                missing = [n for n in bounded if n not in names]
                if missing:
                    raise ValueError(label + " counts the bounded target states {}, which are not goals {}".format(missing, names))

    @staticmethod
    def check_relabel(cfg):
        tcfg = cfg["target"]
        moving = [t["name"] for t in tcfg["states"] if t.get("class", "constant") in ("linear", "sinusoidal")]
        if moving:
            raise ValueError("target states {} move within an episode: a relabelled goal must be constant".format(moving))
        if int(tcfg.get("resample_every", 0) or 0) > 0:
            raise ValueError("target.resample_every > 0 changes the goal within an episode")
        if tcfg.get("on_success", "none") == "new":
            raise ValueError("target.on_success == 'new' changes the goal within an episode")

    def struct(self, step_count_mode=0):
        s = nat.GoalSpecStruct()
        s.n_goals, s.step_count_mode = self.n, int(step_count_mode)
        for i in range(self.n):
            s.k[i], s.mean[i], s.var[i], s.inv_var[i] = self.k[i], self.mean[i], self.var[i], 1.0 / self.var[i]
        return s

    def limits(self, cfg):
        """get_goal_limits (fixed_wing.py:1201-1216): the scaled low / high of the goals' target ranges, float64."""
        low, high = [], []
        for i, name in enumerate(self.names):
            g = [t for t in cfg["target"]["states"] if t["name"] == name][0]
            lo, hi = g["low"], g["high"]
            if g.get("convert_to_radians", False):
                lo, hi = np.radians(lo), np.radians(hi)
            low.append((lo - self.mean[i]) / self.var[i])
            high.append((hi - self.mean[i]) / self.var[i])
        return np.array(low), np.array(high)


def _observe(vec, spec_struct, achieved, desired):
    m = vec._mem
    nat.check(vec._lib, vec._lib.fwg_goal_observe(vec._handle, ctypes.byref(spec_struct), m.ptr(achieved), m.ptr(desired), m.stream()))


def goal_window(vec):
    """W of fwg_goal_window: the largest window_size of the configuration's action-delta factors, 1 when there is none."""
    w = int(vec._lib.fwg_goal_window(vec._handle))
    if w < 0:
        nat.check(vec._lib, w)
    return w


class GoalVecEnv(object):
    """FixedWingAircraftGoal's API over a FixedWingVecEnv.  The goal entries of an observation are views of two [N][4] device
    buffers that one fwg_goal_observe launch fills behind each reset / step: shape [N, G], or [N, L, G] (expanded, no copy) for
    matrix observations, as the reference repeats them."""

    def __init__(self, vec):
        self.vec = vec
        self.num_envs = vec.num_envs
        self.spec = GoalSpec.from_env(vec, reward=False)
        self._obs_spec = self.spec.struct(0)
        m = vec._mem
        self.achieved, self.desired = m.zeros((self.num_envs, 4)), m.zeros((self.num_envs, 4))
        shape = tuple(vec.observation_space.shape)
        G = self.spec.n
        self._length = None if len(shape) == 1 else int(shape[0])
        gshape = (G,) if self._length is None else (self._length, G)
        self.observation_space = DictSpace(dict(desired_goal=Box(-np.inf, np.inf, shape=gshape, dtype="float32"),
                                                achieved_goal=Box(-np.inf, np.inf, shape=gshape, dtype="float32"),
                                                observation=vec.observation_space))
        self.action_space = vec.action_space

    def __getattr__(self, name):   # everything else is the env's (seed, set_curriculum_level, get_attr, close ...)
        return getattr(self.vec, name)

    def _view(self, rows):
        N, G, L = self.num_envs, self.spec.n, self._length
        v = rows[:, :G]
        if L is not None:
            v = v[:, None, :].expand(N, L, G) if hasattr(v, "expand") else np.broadcast_to(v[:, None, :], (N, L, G))
        return self.vec._mem.to_host(v) if self.vec.as_numpy else v

    def _dict(self, obs):
        _observe(self.vec, self._obs_spec, self.achieved, self.desired)
        return dict(observation=obs, achieved_goal=self._view(self.achieved), desired_goal=self._view(self.desired))

    def reset(self, *args, **kwargs):
        return self._dict(self.vec.reset(*args, **kwargs))

    def step(self, actions):
        obs, rew, done, infos = self.vec.step(actions)
        return self._dict(obs), rew, done, infos

    def step_device(self, actions, **kwargs):
        obs, rew, done = self.vec.step_device(actions, **kwargs)
        return self._dict(obs), rew, done

    def get_goal_limits(self):
        return self.spec.limits(self.vec.cfg)

    def compute_reward(self, achieved_goal, desired_goal, info, step_count_mode=0):
        """The reference's compute_reward for m transitions in one launch.  achieved_goal / desired_goal: scaled goals [m, G] (or [G]);
        info: {"step": [m] index of each transition in its episode, "action_window": [m, W, 3] raw actions, W = goal_window(vec), the
        last one the transition's own and the ones before it in the same episode in front of it (entries older than `step` actions
        are not read), "prev_state": [m, G] UNSCALED goal states before the transition (potential form only)}.  Torch device
        tensors or numpy in, the same kind out.  step_count_mode 0 is the reference's counter, 1 step()'s (include/fwgym.h)."""
        vec = self.vec
        m_, lib = vec._mem, vec._lib
        GoalSpec.check_reward(vec.cfg, self.spec.names)
        is_torch = hasattr(achieved_goal, "is_contiguous")
        single = len(tuple(achieved_goal.shape)) == 1
        G, W = self.spec.n, goal_window(vec)

        def rows(x, width, scale=False):
            x = m_.as_device(x).reshape(-1, width)
            out = m_.zeros((x.shape[0], 4))
            if scale:
                mean, var = m_.as_device(self.spec.mean.astype(np.float32)), m_.as_device(self.spec.var.astype(np.float32))
                x = (x - mean) / var
            out[:, :width] = x
            return out

        ach, des = rows(achieved_goal, G), rows(desired_goal, G)
        M = int(ach.shape[0])
        step = m_.as_device(info["step"], "i32").reshape(-1)
        win = m_.as_device(info["action_window"]).reshape(M, W, 3)
        act = m_.zeros((W, M, 4))
        for j in range(W):
            act[j, :, :3] = win[:, j, :]
        prev = rows(info["prev_state"], G, scale=True) if info.get("prev_state", None) is not None else None
        out = m_.zeros((M,))
        spec = self.spec.struct(step_count_mode)
        nat.check(lib, lib.fwg_goal_reward(vec._handle, ctypes.byref(spec), M, m_.ptr(ach), m_.ptr(des),
                                           m_.ptr(prev) if prev is not None else ctypes.c_void_p(), m_.ptr(act), m_.ptr(step), m_.ptr(out),
                                           m_.stream()))
        if not is_torch:
            out = np.asarray(m_.to_host(out))
        return out[0] if single else out


class GoalLog(object):
    """The goal rows of a rollout: achieved / desired [T + 1][N][4], row 0 before step 0 and row t + 1 behind env step t.
    FusedRollout(..., goals=log) launches observe() for it, eagerly and under graph=True; relabel() is HER's "future" strategy over
    the rollout's own buffers."""

    def __init__(self, vec, n_steps):
        self.vec, self.n_steps, self.num_envs = vec, int(n_steps), vec.num_envs
        self.spec = GoalSpec.from_env(vec, reward=True, relabel=True)
        self._obs_spec = self.spec.struct(0)
        m = vec._mem
        self.achieved, self.desired = m.zeros((self.n_steps + 1, self.num_envs, 4)), m.zeros((self.n_steps + 1, self.num_envs, 4))
        self.serial = 0

    def observe(self, row):
        _observe(self.vec, self._obs_spec, self.achieved[row], self.desired[row])

    def relabel(self, buf, p=0.8, seed=0, out=None, step_count_mode=1):
        """fwg_goal_relabel over buf["actions"] / buf["raw_rewards"] / buf["dones"] and this log's rows: every non-terminal
        transition takes, with probability p, the achieved goal of a later row of its episode as its goal, and the reward of that
        goal.  Returns {"desired_goal" [T, N, 4], "rewards" [T, N], "src_row" int32 [T, N]} (`out`: the same dict, reused) and
        advances `serial`, so two calls draw differently.  src_row: the row the goal came from, or -1 kept, -2 terminal, -3 the
        action window reaches before the rollout (include/fwgym.h).  step_count_mode 1: an unrelabelled transition and one
        relabelled to its own goal carry the reward the step gave."""
        vec = self.vec
        m, lib, T, N = vec._mem, vec._lib, self.n_steps, self.num_envs
        if "raw_rewards" not in buf:
            raise ValueError("GoalLog.relabel: the rollout must keep raw rewards (FusedRollout(raw_rewards=True))")
        if tuple(buf["actions"].shape) != (T, N, 3) or tuple(buf["raw_rewards"].shape) != (T, N) or tuple(buf["dones"].shape) != (T, N):
            raise ValueError("GoalLog.relabel: the buffers do not fit {} steps of {} envs with 3 actions".format(T, N))
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError("GoalLog.relabel: p must be a probability")
        if out is None:
            out = {"desired_goal": m.zeros((T, N, 4)), "rewards": m.zeros((T, N)), "src_row": m.zeros((T, N), "i32")}
        spec = self.spec.struct(step_count_mode)
        p_scaled = min(1 << 32, int(round(float(p) * 2.0 ** 32)))
        nat.check(lib, lib.fwg_goal_relabel(vec._handle, ctypes.byref(spec), T, m.ptr(self.achieved), m.ptr(self.desired),
                                            m.ptr(buf["actions"]), m.ptr(buf["raw_rewards"]), m.ptr(buf["dones"]),
                                            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_uint32(self.serial & 0xFFFFFFFF),
                                            ctypes.c_uint64(p_scaled), m.ptr(out["desired_goal"]), m.ptr(out["rewards"]),
                                            m.ptr(out["src_row"]), m.stream()))
        self.serial += 1
        return out
