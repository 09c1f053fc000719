"""HindsightReplay -- a hindsight experience replay buffer on the device: what an off-policy learner puts between a GoalVecEnv
(gym_fixed_wing.goal) and its update.

GoalLog.relabel relabels one rollout once, in place and in rollout order.  An off-policy learner keeps many rollouts, draws
minibatches uniformly over all of them, and wants a fresh hindsight goal -- with that goal's reward -- every time a transition is
drawn.  With torch indexing that is six or seven advanced-indexing gathers per minibatch, a scan for each sample's episode end and
a compute_reward call; here it is one launch per stored rollout (fwg_replay_index: the episode end of every transition) and one
launch per minibatch (fwg_replay_sample: the draw, the goal gather, the reward of the new goal and the row gathers);
csrc/fwgym_replay.h, include/fwgym.h "Hindsight replay".

    replay = HindsightReplay(vec, n_steps, slots, strategy="future", p=0.8)
    replay.add_rollout(rollout)            # a FusedRollout(vec, actor, n_steps, raw_rewards=True, goals=log)
    replay.add(obs, last_obs, actions, raw_rewards, dones, log)   # ... or step-major buffers of a loop of one's own
    batch = replay.sample(4096)            # {"observation", "next_observation", "action", "achieved_goal", "desired_goal",
                                           #  "reward", "done", "index"}: device tensors

Nothing of the env, the rollout or a learner changes while no replay is attached: it owns its buffers and launches only from its
own calls."""
import ctypes

from . import _native as nat
from .goal import GoalSpec

STRATEGIES = ("future", "final", "episode")


def without_goal_targets(cfg):
    """A copy of the configuration dict whose observation.states no longer list the targets of the goal states (the entries
    HindsightReplay refuses): the goal then reaches a learner through `desired_goal` only.  The result is another observation
    layout, so it is no build-time preset (FixedWingVecEnv specialises a kernel for it, or runs the generic one)."""
    import copy
    cfg = copy.deepcopy(cfg)
    names = [g["name"] for g in cfg["observation"].get("goals", None) or []]
    cfg["observation"]["states"] = [s for s in cfg["observation"]["states"] if not (s.get("type") == "target" and s.get("name") in names)]
    return cfg


class HindsightReplay(object):
    """`slots` rollouts of `n_steps` steps of every env of `vec`, slot-major on the device; the oldest slot is overwritten.

    strategy: where a relabelled transition takes its goal from -- "future": a row behind it in its episode (HER's default);
    "final": the last row of its episode that the slot holds; "episode": any row of its episode in the slot.  A goal never comes
    from another slot, nor from across a done.  p: the share of the eligible transitions that are relabelled (stable-baselines'
    n_sampled_goal = 4 is p = 0.8).  Terminal transitions keep their goal (under auto-reset the goal they achieved is not in the
    buffer), and so do the first W - 1 transitions of a slot whose action window reaches before it (W: goal_window(vec)).

    The reward of a relabelled transition is the reference's compute_reward under step()'s step counter (step_count_mode 1: a
    transition relabelled to the goal it had carries the reward the step gave); every other transition carries its raw reward.

    OBSERVATIONS ARE NOT REWRITTEN.  stable-baselines' HER does not rewrite them either: it stores observation and goals side by
    side and relabels the goal entries only.  An observation vector that itself holds the target of a goal state (an
    observation.states entry of type "target" naming a goal) would contradict a relabelled goal, so such a configuration is refused
    with the entry's name; target_observations="stale" accepts it knowingly (the learner then has to ignore those words).  The
    stored observations are the caller's: add_rollout() stores them as the FusedRollout holds them, that is, normalised by the
    head's statistics AT COLLECTION TIME.

    Under auto-reset `next_observation` and `achieved_goal` of a terminal sample show the next episode; `done` says so.

    sample() is an eager call: `serial`, which makes every call draw differently, travels by value, so capturing it into a graph
    would replay one minibatch -- out of scope here."""

    def __init__(self, vec, n_steps, slots, strategy="future", p=0.8, seed=0, target_observations="refuse"):
        if strategy not in nat.REPLAY_STRATEGIES:
            raise ValueError("HindsightReplay: unknown strategy '{}' (one of {})".format(strategy, list(STRATEGIES)))
        if target_observations not in ("refuse", "stale"):
            raise ValueError("HindsightReplay: target_observations must be 'refuse' or 'stale'")
        if int(n_steps) < 1 or int(slots) < 1:
            raise ValueError("HindsightReplay: n_steps and slots must be positive")
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError("HindsightReplay: p must be a probability")
        self.vec, self.n_steps, self.slots, self.num_envs = vec, int(n_steps), int(slots), vec.num_envs
        self.spec = GoalSpec.from_env(vec, reward=True, relabel=True)
        stale = [s for s in vec.cfg["observation"]["states"] if s.get("type") == "target" and s.get("name") in self.spec.names]
        if stale and target_observations != "stale":
            raise ValueError("HindsightReplay: observation.states entry {} (type 'target', value '{}') shows the target of goal '{}': the "
                             "observation of a relabelled sample would contradict its goal -- take the entry out of the observation, or "
                             "pass target_observations='stale'".format(vec.cfg["observation"]["states"].index(stale[0]),
                                                                       stale[0].get("value"), stale[0]["name"]))
        self.obs_dim = int(vec.obs_dim)
        if not 1 <= self.obs_dim <= nat.REPLAY_MAX_OBS:
            raise ValueError("HindsightReplay: observations of {} words, the sample kernel takes 1 .. {}".format(self.obs_dim, nat.REPLAY_MAX_OBS))
        self.strategy, self.p, self.seed = strategy, float(p), int(seed)
        self.p_scaled = min(1 << 32, int(round(self.p * 2.0 ** 32)))
        self._spec = self.spec.struct(1)
        m, K, T, N, D = vec._mem, self.slots, self.n_steps, self.num_envs, self.obs_dim
        self.obs = m.zeros((K, T + 1, N, D))
        self.actions, self.raw_rewards = m.zeros((K, T, N, 3)), m.zeros((K, T, N))
        self.dones, self.ep_end = m.zeros((K, T, N), "u8"), m.zeros((K, T, N), "i32")
        self.achieved, self.desired = m.zeros((K, T + 1, N, 4)), m.zeros((K, T + 1, N, 4))
        self.count = 0    # rollouts added so far (slot of the next one: count % slots)
        self.serial = 0   # sample() calls so far
        v = self._view = nat.ReplayView()
        v.n_slots, v.n_filled, v.n_steps, v.n_envs, v.obs_words = K, 0, T, N, D
        for name in ("obs", "actions", "raw_rewards", "dones", "ep_end", "achieved", "desired"):
            setattr(v, name, m.ptr(getattr(self, name)).value)

    @property
    def filled(self):
        return min(self.count, self.slots)

    def __len__(self):
        return self.filled * self.n_steps * self.num_envs

    def add(self, obs, last_obs, actions, raw_rewards, dones, log):
        """Copies one step-major rollout into slot count % slots and indexes its episodes: obs [T, N, D] the observation each step
        was taken from, last_obs [N, D] the one behind the last step, actions [T, N, 3], raw_rewards [T, N], dones uint8 [T, N],
        log: the GoalLog (or anything with .achieved / .desired [T + 1, N, 4]) that observed the rollout.  Returns the slot."""
        T, N, D = self.n_steps, self.num_envs, self.obs_dim
        want = (("obs", obs, (T, N, D)), ("last_obs", last_obs, (N, D)), ("actions", actions, (T, N, 3)), ("raw_rewards", raw_rewards, (T, N)),
                ("dones", dones, (T, N)), ("log.achieved", log.achieved, (T + 1, N, 4)), ("log.desired", log.desired, (T + 1, N, 4)))
        for name, x, shape in want:
            if tuple(x.shape) != shape:
                raise ValueError("HindsightReplay.add: {} has shape {}, a rollout of {} steps of {} envs needs {}".format(
                    name, tuple(x.shape), T, N, shape))
        k = self.count % self.slots
        self.obs[k][:T][...] = obs
        self.obs[k][T][...] = last_obs
        self.actions[k][...] = actions
        self.raw_rewards[k][...] = raw_rewards
        self.dones[k][...] = dones
        self.achieved[k][...] = log.achieved
        self.desired[k][...] = log.desired
        m, lib = self.vec._mem, self.vec._lib
        nat.check(lib, lib.fwg_replay_index(T, N, m.ptr(self.dones[k]), m.ptr(self.ep_end[k]), m.stream()))
        self.count += 1
        return k

    def add_rollout(self, rollout):
        """add() for a FusedRollout(vec, actor, n_steps, raw_rewards=True, goals=log) that has just run: its buffers, the head's
        current observation as the last row, and its log.  The observations are the NORMALISED ones the rollout holds."""
        if getattr(rollout, "goals", None) is None or "raw_rewards" not in rollout.buf:
            raise ValueError("HindsightReplay.add_rollout: the rollout must keep raw rewards and goal rows "
                             "(FusedRollout(raw_rewards=True, goals=log))")
        b = rollout.buf
        return self.add(b["obs"], rollout.cur["obs"], b["actions"], b["raw_rewards"], b["dones"], rollout.goals)

    def empty_batch(self, batch_size):
        m, B, D = self.vec._mem, int(batch_size), self.obs_dim
        return {"observation": m.zeros((B, D)), "next_observation": m.zeros((B, D)), "action": m.zeros((B, 3)),
                "achieved_rows": m.zeros((B, 4)), "desired_rows": m.zeros((B, 4)), "reward": m.zeros((B,)), "done": m.zeros((B,), "u8"),
                "index": m.zeros((B, 4), "i32")}

    def sample(self, batch_size, out=None):
        """One minibatch, drawn uniformly (with replacement) over the stored transitions and relabelled in the same launch.
        Returns {"observation" [B, D], "next_observation" [B, D], "action" [B, 3], "achieved_goal" [B, G] (behind the transition),
        "desired_goal" [B, G], "reward" [B], "done" uint8 [B], "index" int32 [B, 4] = (slot, step, env, src)}; src: the row the goal
        came from, or -1 kept, -2 terminal, -3 the action window reaches before the slot.  The goals are views of 4-word rows
        ("achieved_rows" / "desired_rows").  `out`: a dict this call returned for the same batch size, reused.  Advances `serial`."""
        B = int(batch_size)
        if self.count < 1:
            raise ValueError("HindsightReplay.sample: the buffer is empty")
        if B < 1:
            raise ValueError("HindsightReplay.sample: the batch size must be positive")
        if out is None:
            out = self.empty_batch(B)
        elif tuple(out["observation"].shape) != (B, self.obs_dim):
            raise ValueError("HindsightReplay.sample: `out` was made for another batch size")
        m, lib, G = self.vec._mem, self.vec._lib, self.spec.n
        self._view.n_filled = self.filled
        nat.check(lib, lib.fwg_replay_sample(self.vec._handle, ctypes.byref(self._spec), ctypes.byref(self._view), nat.REPLAY_STRATEGIES[self.strategy],
                                             B, ctypes.c_uint64(self.seed & (2 ** 64 - 1)), ctypes.c_uint32(self.serial & 0xFFFFFFFF),
                                             ctypes.c_uint64(self.p_scaled), m.ptr(out["observation"]), m.ptr(out["next_observation"]),
                                             m.ptr(out["action"]), m.ptr(out["achieved_rows"]), m.ptr(out["desired_rows"]), m.ptr(out["reward"]),
                                             m.ptr(out["done"]), m.ptr(out["index"]), m.stream()))
        self.serial += 1
        out["achieved_goal"], out["desired_goal"] = out["achieved_rows"][:, :G], out["desired_rows"][:, :G]
        return out
