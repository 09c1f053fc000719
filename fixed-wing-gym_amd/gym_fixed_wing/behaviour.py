"""BehaviourHead / HindsightCollector -- the behaviour policy of an offpolicy.DDPG as ONE HIP launch per act, and an exploration
rollout for replay.HindsightReplay as 2 T + 1 launches, eagerly or as one replayed graph (csrc/fwgym_behaviour.h; include/fwgym.h
"Behaviour head").

    agent = DDPG(vec.obs_dim, 3, update="hip")
    collector = HindsightCollector(vec, agent, n_steps=64, graph=True, noise=0.2, random_eps=0.3)
    vec.reset()
    collector.run()                        # T env steps of every env under pi(o, g) + exploration
    replay.add_rollout(collector)          # unchanged: it reads .buf, .cur["obs"] and .goals
    agent.update(replay.sample(4096))      # update="hip": the next run() acts on the new weights, no copy, no recapture

One launch (fwg_behaviour_act) computes the goal rows of the env's state (what fwg_goal_observe writes, into the rollout's GoalLog),
gathers [obs | goal], copies the observation rows into the rollout, runs the actor from the learner's flat parameter vector in place,
draws the exploration noise on the device (Philox, a per-env counter in device memory) and files the previous step's done flags.

Nothing of the env, the rollout, the replay buffer or a learner changes while neither class is in use: they own their buffers and
launch only from their own calls."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from .goal import GoalLog
from .offpolicy import GOAL_STRIDE, MAX_WIDTH


def _ptr(x):
    """Device pointer of a torch tensor or (host emulation) of a numpy array; None -> NULL."""
    if x is None:
        return ctypes.c_void_p()
    if isinstance(x, torch.Tensor):
        return ctypes.c_void_p(int(x.data_ptr()))
    return ctypes.c_void_p(x.ctypes.data)


def _checked(who, name, x, shape, kind, device):
    """The kernel reads and writes through raw pointers: anything but a contiguous buffer of the right shape, type and device is
    refused by name."""
    dt = str(x.dtype).replace("torch.", "")
    ok = tuple(x.shape) == tuple(shape) and dt == kind
    if ok and isinstance(x, torch.Tensor):
        ok = x.is_contiguous() and x.device.type == device.type and (device.type != "cuda" or x.device == device)
    elif ok:
        ok = isinstance(x, np.ndarray) and bool(x.flags["C_CONTIGUOUS"]) and device.type == "cpu"
    if not ok:
        raise ValueError("{}: {} must be a contiguous {} buffer of shape {} on {} (it is {} {})".format(
            who, name, kind, tuple(shape), device, dt, tuple(getattr(x, "shape", ()))))
    return x


def eps_scaled(random_eps):
    """HindsightReplay.p_scaled's rule: min(2^32, round(eps 2^32)), compared with a 32-bit Philox word as `x < eps_scaled`."""
    if not 0.0 <= float(random_eps) <= 1.0:
        raise ValueError("random_eps must be a probability, it is {!r}".format(random_eps))
    return min(1 << 32, int(round(float(random_eps) * 2.0 ** 32)))


class BehaviourHead(object):
    """pi(o, g) of `agent` (an offpolicy.DDPG) with exploration for `num_envs` envs: env i draws the Philox stream of
    (seed, env_id_base + i), whatever the batch it is part of, so shards of one population explore as the whole would.

    noise: std of the Gaussian noise added to pi (then clipped to [-1, 1]); random_eps: the probability, per env and act, of a
    uniform action in [-1, 1)^A instead (stable-baselines HER's random_eps).  Both live in a small device buffer: set_noise()
    changes them with one copy, also between replays of a captured collector.

    The weights.  update="hip": the head reads agent.updater.flat in place -- an update, a load() or load_params() is seen by the
    next act with no copy.  update="torch": the head owns a copy of the actor's parameters and refresh() packs actor.parameters()
    into it; call refresh() after every agent.update() / agent.load() whose weights the next act should use (the constructor has
    called it once).  Without it the head keeps acting on the weights of the last refresh().  The copy keeps its address, so a
    captured collector needs no recapture either way.

    The seed travels by value: reseed() is refused once a graph=True collector has captured this head's launches."""

    def __init__(self, agent, num_envs, seed=0, env_id_base=0, noise=0.2, random_eps=0.0, _lib=None):
        self.agent, self.num_envs = agent, int(num_envs)
        if self.num_envs < 1:
            raise ValueError("BehaviourHead: num_envs must be positive, it is {}".format(num_envs))
        self.device = torch.device(agent.device)
        self.obs_dim, self.goal_dim, self.act_dim = agent.obs_dim, agent.goal_dim, agent.act_dim
        D, G, A = self.obs_dim, self.goal_dim, self.act_dim
        if D + G + A > MAX_WIDTH:
            raise ValueError("BehaviourHead: obs_dim + goal_dim + act_dim = {} exceeds {} (obs_dim {}, goal_dim {}, act_dim {}): one LDS "
                             "tile row holds a network's input".format(D + G + A, MAX_WIDTH, D, G, A))
        self.actor_params = 64 * (D + G) + 64 + 64 * 64 + 64 + A * 64 + A
        hip = agent.update_path == "hip"
        self._lib = _lib if _lib is not None else (agent.updater._lib if hip else nat.load_library())
        if hip:
            assert agent.updater.actor_params == self.actor_params
            self.params = agent.updater.flat    # (a view of nothing: the learner's own vector, its first PA words the actor's)
        else:
            self.params = torch.zeros(self.actor_params, device=self.device)
        self._own_params = not hip
        self.draws = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)   # uint32 counters, as bits
        self.noise_params = torch.zeros(nat.BEHAVIOUR_NOISE_WORDS, dtype=torch.int32, device=self.device)
        self.seed, self.env_id_base = int(seed), int(env_id_base)
        self._captured = False
        self.set_noise(noise, random_eps)
        self.refresh()

    def refresh(self):
        """update="torch": packs actor.parameters() into the head's own buffer (see the class docstring for when).  update="hip":
        nothing to do."""
        if self._own_params:
            with torch.no_grad():
                self.params.copy_(torch.cat([p.detach().reshape(-1) for p in self.agent.actor.parameters()]))

    def set_noise(self, noise, random_eps):
        """sigma and eps_scaled on the device: one small copy on the current stream, never a recapture."""
        if not float(noise) >= 0.0 or not np.isfinite(float(noise)):
            raise ValueError("BehaviourHead.set_noise: noise must be a finite std >= 0, it is {!r}".format(noise))
        e = eps_scaled(random_eps)
        words = np.array([np.array(noise, dtype=np.float32).view(np.uint32), e & 0xFFFFFFFF, e >> 32, 0], dtype=np.uint32)
        self.noise_params.copy_(torch.from_numpy(words.view(np.int32)))
        self.noise, self.random_eps = float(noise), float(random_eps)

    def reseed(self, seed):
        """Another stream from its beginning: the seed, and every env's draw counter back to 0."""
        if self._captured:
            raise RuntimeError("BehaviourHead.reseed: a captured collector holds this head's seed by value -- reseed before building "
                               "the graph=True collector")
        self.seed = int(seed)
        self.draws.zero_()

    def close(self):
        """Releases the head's device buffers (the learner's parameter vector is the learner's)."""
        self.params = self.draws = self.noise_params = None

    def _stream(self):
        if self.device.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return ctypes.c_void_p()

    def _launch(self, env, spec, obs, goal_rows, achieved, desired, obs_out, action, done_in, done_out, deterministic):
        if self.params is None:
            raise RuntimeError("BehaviourHead: the head is closed")
        lib = self._lib
        nat.check(lib, lib.fwg_behaviour_act(env, spec, self.num_envs, self.obs_dim, self.goal_dim, self.act_dim, _ptr(self.params), _ptr(obs),
                                             _ptr(goal_rows), _ptr(achieved), _ptr(desired), _ptr(obs_out), _ptr(action), _ptr(done_in),
                                             _ptr(done_out), _ptr(self.draws), _ptr(self.noise_params),
                                             ctypes.c_uint64(self.seed & (2 ** 64 - 1)), ctypes.c_uint32(self.env_id_base & 0xFFFFFFFF),
                                             int(bool(deterministic)), self._stream()))

    def act(self, obs, desired_rows, out=None, deterministic=False):
        """The env-less form: obs float32 [N, D], desired_rows float32 [N, 4] (goal rows as HindsightReplay.sample's "desired_rows"
        or a GoalLog's), both on the head's device -> actions [N, A] (`out`, or a new buffer of obs' kind).  Advances every env's
        draw counter unless `deterministic`."""
        N, D, A = self.num_envs, self.obs_dim, self.act_dim
        _checked("BehaviourHead.act", "obs", obs, (N, D), "float32", self.device)
        _checked("BehaviourHead.act", "desired_rows", desired_rows, (N, GOAL_STRIDE), "float32", self.device)
        if out is None:
            out = torch.zeros((N, A), device=self.device) if isinstance(obs, torch.Tensor) else np.zeros((N, A), dtype=np.float32)
        _checked("BehaviourHead.act", "out", out, (N, A), "float32", self.device)
        self._launch(None, None, obs, desired_rows, None, None, None, out, None, None, deterministic)
        return out

    def act_env(self, vec, spec_struct, achieved, desired, obs_out, action, done_out=None, deterministic=False):
        """The env form, as HindsightCollector issues it: the goal rows of vec's state into achieved / desired [N, 4], vec's
        observation into obs_out, the actions into `action`, vec's done flags into done_out (None: not filed)."""
        N, D, A = self.num_envs, self.obs_dim, self.act_dim
        who = "BehaviourHead.act_env"
        if vec.num_envs != N or vec.obs_dim != D:
            raise ValueError("{}: the env has {} envs of {} observation words, the head {} of {}".format(who, vec.num_envs, vec.obs_dim, N, D))
        for name, x, shape, kind in (("achieved", achieved, (N, 4), "float32"), ("desired", desired, (N, 4), "float32"),
                                     ("obs_out", obs_out, (N, D), "float32"), ("action", action, (N, A), "float32"),
                                     ("done_out", done_out, (N,), "uint8")):
            if x is not None:
                _checked(who, name, x, shape, kind, self.device)
        self._launch(vec._handle, ctypes.byref(spec_struct), vec._obs, None, achieved, desired, obs_out, action,
                     None if done_out is None else vec._done, done_out, deterministic)


class HindsightCollector(object):
    """Exploration rollouts of `n_steps` steps of every env of `vec` (a FixedWingVecEnv with observation.goals) under `agent`'s
    behaviour policy, in the structure of rollout.FusedRollout: the act behind env step t writes rollout slice t + 1 and dones[t],
    the last act writes `cur`.  Per rollout T launches of fwg_step (its rewards go to raw_rewards[t]) and T + 1 of the head -- no
    goal observation, copy or cat launches: the head fills goals.achieved[t] / goals.desired[t] and buf["obs"][t] itself.

        buf    {"obs" [T, N, D], "actions" [T, N, 3], "raw_rewards" [T, N], "dones" uint8 [T, N]}
        cur    {"obs" [N, D], "actions" [N, 3]}: the observation behind the last step (a replay's last row) and the head's action
               for it.  The next rollout acts on that observation AGAIN, with a new draw, into its slice 0: `cur["actions"]` is
               never executed
        goals  the GoalLog of the rollout (HindsightReplay.add_rollout(collector) reads buf, cur["obs"] and goals)

    head: a BehaviourHead of this agent and env count (default: a new one from **head_kw: seed, env_id_base, noise, random_eps).
    graph=True captures one rollout into one graph on one stream and run() replays it (n_steps must be even); the two warm-up env
    steps of the capture are env steps like any other, their rewards and done flags are kept in `warmup` ([2, N] each).  An
    attached FlightRecorder records from inside vec.step_device, so the capture holds its launches: attach it before building the
    collector, as for any graphed rollout.

    Refused by name: row-log envs (the head reads the dense observation batch), odd n_steps under graph=True, an agent or a head
    whose dimensions are not the env's, and whatever GoalLog refuses (no goals, goals whose substituted reward is not defined)."""

    def __init__(self, vec, agent, n_steps, head=None, graph=False, **head_kw):
        self.vec, self.agent, self.n_steps = vec, agent, int(n_steps)
        who = "HindsightCollector"
        if self.n_steps < 1:
            raise ValueError("{}: n_steps must be positive, it is {}".format(who, n_steps))
        if getattr(vec, "obs_log_rows", 0):
            raise ValueError("{}: the env writes a row log (obs_log_rows {}): the behaviour head reads the dense observation batch -- "
                             "build the env with obs_layout='dense'".format(who, vec.obs_log_rows))
        if graph and self.n_steps % 2:
            raise ValueError("{}(graph=True): n_steps must be even (graph mode double-buffers the step counter), it is {}".format(who, n_steps))
        self.goals = GoalLog(vec, self.n_steps)
        N, D, G = vec.num_envs, vec.obs_dim, self.goals.spec.n
        if (agent.obs_dim, agent.goal_dim, agent.act_dim) != (D, G, 3):
            raise ValueError("{}: the agent has (obs_dim, goal_dim, act_dim) = {}, the env needs {}".format(
                who, (agent.obs_dim, agent.goal_dim, agent.act_dim), (D, G, 3)))
        if head is None:
            head = BehaviourHead(agent, N, **head_kw)
        elif head_kw:
            raise ValueError("{}: pass either head or the head's arguments {}".format(who, sorted(head_kw)))
        if head.agent is not agent or head.num_envs != N:
            raise ValueError("{}: head belongs to another agent or has num_envs {} (the env has {})".format(who, head.num_envs, N))
        self.head = head
        m = vec._mem
        self.buf = {"obs": m.zeros((self.n_steps, N, D)), "actions": m.zeros((self.n_steps, N, 3)), "raw_rewards": m.zeros((self.n_steps, N)),
                    "dones": m.zeros((self.n_steps, N), "u8")}
        self.cur = {"obs": m.zeros((N, D)), "actions": m.zeros((N, 3))}
        self.warmup = None
        self._spec = self.goals.spec.struct(0)
        self._graph = None
        if graph:
            self._capture()

    def _act(self, row, slot, done_out=None):
        """The head on the env's current state: goal rows into row `row` of the log, observation and action into `slot`."""
        g = self.goals
        self.head.act_env(self.vec, self._spec, g.achieved[row], g.desired[row], slot["obs"], slot["actions"], done_out)

    def _body(self):
        buf, cur, T = self.buf, self.cur, self.n_steps
        self._act(0, {"obs": buf["obs"][0], "actions": buf["actions"][0]})
        for t in range(T):
            self.vec.step_device(buf["actions"][t], reward_out=buf["raw_rewards"][t])
            nxt = cur if t == T - 1 else {"obs": buf["obs"][t + 1], "actions": buf["actions"][t + 1]}
            self._act(t + 1, nxt, buf["dones"][t])

    def warm_up(self):
        """The capture's two warm-up env steps (three head launches, every kernel of the body launched once): acts into `cur` and
        goal row 0, rewards and done flags into `warmup`.  graph=True runs it once before the capture; an eager collector that is to
        reproduce a captured one calls it at the same point."""
        m, N = self.vec._mem, self.vec.num_envs
        warm = self.warmup = (m.zeros((2, N)), m.zeros((2, N), "u8"))
        self._act(0, self.cur)
        for i in range(2):
            self.vec.step_device(self.cur["actions"], reward_out=warm[0][i])
            self._act(0, self.cur, warm[1][i])
        return warm

    def _capture(self):
        vec = self.vec
        dev = vec._obs.device
        vec.set_graph_mode(True)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # warm-up outside capture
            self.warm_up()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        self._parity = vec.capture_begin(self.n_steps)
        with torch.cuda.graph(graph):
            self._body()
        vec.capture_end()
        self.head._captured = True
        self._graph = graph

    def run(self):
        """One rollout from the env's current state (after vec.reset(), or where the last one ended) -> buf."""
        if self._graph is not None:
            self.vec.replay_check(self._parity)
            self._graph.replay()
            self.vec.note_replayed_steps(self.n_steps)
        else:
            self._body()
        return self.buf
