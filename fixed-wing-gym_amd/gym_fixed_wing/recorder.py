"""FlightRecorder -- the episode history of a few envs of a FixedWingVecEnv, kept on the device.

The reference's training callback renders one training episode every few minutes
(examples/train_rl_controller.py:31-110: env.env_method("render", indices=0, mode="plot", show=False, save_path=...)); its env
keeps that episode's history on the host, one append per step (fixed_wing.py:338-437).  A training rollout here is a replayed
hipGraph with no host read inside, so the history is kept by a small kernel launched behind every env step
(csrc/fwgym_record.h, include/fwgym.h "Flight recorder"): per tracked env two slabs of 128-byte rows, the episode in progress and
the last completed one.  This module owns the buffers, decodes a slab into the single-env class's `simulator.state[*].history` /
`history` structures and draws the reference's figure from them (the plotting and save_history bodies below serve
FixedWingAircraft too).

ONE difference from the single-env class: under auto-reset the step that ends an episode leaves the NEXT episode's reset state
in the arena, so the terminal step carries its action, reward and termination but no state sample -- `Episode.states` and the
target / error / goal lists have `length` entries (the reset sample and one per step but the last), as many as
`history["action"]` and one fewer than the single-env class keeps for such an episode.  With auto_reset off an episode that ends by
"steps" / "success" has its terminal state, and one that ends in a simulator failure has none, exactly as the single-env class.
"""
import os

import numpy as np

from . import _native as nat

_RECORDED = ["roll", "pitch", "yaw", "omega_p", "omega_q", "omega_r", "position_n", "position_e", "position_d",
             "velocity_u", "velocity_v", "velocity_w", "Va", "alpha", "beta", "elevator", "aileron", "throttle"]
_ACTUATORS = ("elevator", "aileron", "throttle")
# word of a recorder row that holds each recorded state (elevator / aileron: computed from the elevon words 13 / 14)
_ROW_WORD = {"roll": 16, "pitch": 17, "yaw": 18, "omega_p": 4, "omega_q": 5, "omega_r": 6, "position_n": 7, "position_e": 8,
             "position_d": 9, "velocity_u": 10, "velocity_v": 11, "velocity_w": 12, "Va": 19, "alpha": 20, "beta": 21, "throttle": 15}
W_TARGET, W_ACTION, W_REWARD, W_STEPS, W_DONE = 22, 25, 28, 29, 30


# ----------------------------------------------------------------------------------------------------------------------
# shared with the single-env class (gym_fixed_wing.fixed_wing.FixedWingAircraft)
# ----------------------------------------------------------------------------------------------------------------------
def constrained_command(cfg, env_config, action):
    """What PyFly stores in simulator.state[actuator].history["command"] (read by the reference at fixed_wing.py:828 and
    :1110): the inputs after action scaling (fixed_wing.py:349-354,439-459), the value limits of elevator / aileron / throttle
    and of the two elevons, mapped back to elevator / aileron -- the same arithmetic the step kernel applies
    (csrc/fwgym_physics.h constrain_commands)."""
    ec = env_config
    a = np.asarray(action, dtype=np.float64).reshape(3)
    if cfg["action"].get("scale_space", False):
        lo, hi = cfg["action"].get("scale_low", -1), cfg["action"].get("scale_high", 1)
        to_lo, to_hi = ec.action_scale_to_low, ec.action_scale_to_high
        a = (to_hi - to_lo) * (np.clip(a, lo, hi) - lo) / (hi - lo) + to_lo

    def lim(x, name):
        v = ec.state[name]
        if getattr(v, "value_min", None) is not None:
            x = max(x, v.value_min)
        if getattr(v, "value_max", None) is not None:
            x = min(x, v.value_max)
        return x
    e, al, t = lim(a[0], "elevator"), lim(a[1], "aileron"), lim(a[2], "throttle")
    er, el = lim(e - al, "elevon_right"), lim(e + al, "elevon_left")
    return {"elevator": 0.5 * (er + el), "aileron": 0.5 * (el - er), "throttle": t}


def target_error(env_config, name, value, target):
    """Error of one target state as the single-env class reports it (wrapped for angles)."""
    if env_config.state[name].wrap:
        d = (value - target + np.pi) % (2 * np.pi) - np.pi
        return d + 2 * np.pi if d < -np.pi else d
    return target - value


def goal_status(env_config, values, targets):
    """{state: |error| <= bound, ..., "all": ...} for the states that have a bound (fixed_wing.py:993-1011)."""
    st = {}
    for name, props in env_config.target_props_init["states"].items():
        if props.get("bound", None) is not None:
            b = np.radians(props["bound"]) if props.get("convert_to_radians", False) else props["bound"]
            st[name] = bool(np.abs(target_error(env_config, name, values[name], targets[name])) <= b)
    st["all"] = all(st.values())
    return st


def plot_episode(cfg, env_config, states, history, mode="plot", show=True, close=True, block=False, save_path=None):
    """The reference's episode figure (fixed_wing.py:572-652) from `states` (name -> history list, or {"value", "command"} for
    the actuators) and `history` ({"action", "reward", "target", "goal"}).  Returns (result, viewer): the figure when it is kept
    open (close=False, mode "plot"), else None; viewer = {"fig", "gs"} while the figure lives."""
    if mode not in ("plot", "rgb_array"):
        if mode == "animation":
            raise NotImplementedError
        raise ValueError("Unexpected value {} for mode".format(mode))
    import matplotlib
    if not show:
        matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    import matplotlib.gridspec
    rcfg = cfg["render"]
    goal_enabled = env_config.goal_enabled
    groups = [("roll", "pitch"), ("Va",), ("omega_p", "omega_q", "omega_r"), ("elevator", "aileron", "throttle")]
    extra = int(bool(rcfg["plot_action"])) + int(bool(rcfg["plot_reward"]))
    fig = plt.figure(figsize=(9, 16))
    gs = matplotlib.gridspec.GridSpec(len(groups) + extra, 1)
    for gi, names in enumerate(groups):
        ax = plt.subplot(gs[gi, 0])
        for n in names:
            h = states[n]
            y = h["value"] if isinstance(h, dict) else h
            line, = ax.plot(range(len(y)), y, label=n)
            if rcfg["plot_target"] and n in history["target"]:
                tgt = np.array(history["target"][n])
                ax.plot(range(len(tgt)), tgt, "--", color=line.get_color(), label=n + " target")
                if rcfg["plot_goal"] and goal_enabled and n in history["goal"]:
                    p = env_config.target_props_init["states"][n]
                    b = np.radians(p["bound"]) if p.get("convert_to_radians", False) else p["bound"]
                    ok = np.array(history["goal"][n], dtype=bool)[:len(tgt)]
                    ax.fill_between(range(len(tgt)), tgt - b, tgt + b, where=ok, alpha=0.2, color=line.get_color())
        ax.legend(loc="upper right")
    if rcfg["plot_action"]:
        ax = plt.subplot(gs[-extra, 0], title="Actions")
        y = np.array(history["action"]).reshape(-1, 3)
        for i, a in enumerate(cfg["action"]["states"]):
            ax.plot(range(len(y)), y[:, i], label=a["name"])
        ax.legend()
    if rcfg["plot_reward"]:
        ax = plt.subplot(gs[-1, 0], title="Reward")
        ax.plot(range(len(history["reward"])), history["reward"])
    viewer = {"fig": fig, "gs": gs}
    if save_path is not None:
        d = os.path.dirname(save_path)
        if d and not os.path.isdir(d):
            os.makedirs(d)
        ext = os.path.splitext(save_path)[1]
        plt.savefig(save_path, bbox_inches="tight", **({"format": ext[1:]} if ext else {}))
    if mode == "rgb_array":
        return None, viewer
    if show:
        plt.show(block=block)
    if close:
        plt.close(fig)
        return None, None
    return fig, viewer


def history_dict(cfg, env_config, states, history, names, save_targets=True):
    """What save_history writes (reference fixed_wing.py:654-672): state histories (+ '<state>_target' entries)."""
    res = {}
    for s in ([names] if isinstance(names, str) else names):
        h = states[s]
        res[s] = list(h["value"] if isinstance(h, dict) else h)
    if save_targets:
        for s in history["target"]:
            if s in res:
                res[s + "_target"] = history["target"][s]
    return res


def save_history_file(cfg, env_config, states, history, path, names, save_targets=True):
    np.save(path, history_dict(cfg, env_config, states, history, names, save_targets))


# ----------------------------------------------------------------------------------------------------------------------
class Episode(object):
    """One recorded episode, decoded.  `rows` is the raw slab ([length + 1][32] float32, include/fwgym.h "Flight recorder");
    `full[t]`: row t carries a state sample (every row but, possibly, the terminal one)."""

    def __init__(self, vec, rows, termination_code, episode_index, overflowed, complete):
        cfg, ec = vec.cfg, vec.env_config
        self.rows = rows
        bits = rows.view(np.int32)
        n = rows.shape[0]
        self.length = n - 1
        self.complete = bool(complete)
        self.termination = nat.term_name(termination_code) if complete else None
        self.episode_index = int(episode_index)
        self.overflowed = bool(overflowed)
        done = (bits[:, W_DONE] & 0xFF) != 0
        term = (bits[:, W_DONE] >> 8) & 0xFF
        ended_ok = (term == nat.TERM_STEPS) | (term == nat.TERM_SUCCESS)
        self.full = ~done | (ended_ok & (not vec.auto_reset))
        failed = done & ~ended_ok
        self.consistent = bool(np.all((bits[self.full, W_STEPS] & 0xFFFF) == np.arange(n)[self.full]))
        names = list(vec.target_names)
        half = np.float32(0.5)

        def column(name):
            if name == "elevator":
                return half * (rows[:, 13] + rows[:, 14])      # (the float32 expressions of FixedWingVecEnv.field)
            if name == "aileron":
                return half * (rows[:, 14] - rows[:, 13])
            return rows[:, _ROW_WORD[name]]
        cols = {name: column(name) for name in _RECORDED}
        self.states = {}
        for name in _RECORDED:
            vals = [float(v) for v in cols[name][self.full]]
            self.states[name] = {"value": vals, "command": []} if name in _ACTUATORS else vals
        hist = {"action": [], "reward": [], "target": {k: [] for k in names}, "error": {k: [] for k in names}}
        if ec.goal_enabled:
            hist["goal"] = None
        prev_target = None
        for t in range(n):
            if t > 0:
                action = rows[t, W_ACTION:W_ACTION + 3].astype(np.float64)
                hist["action"].append(action)
                for a, v in constrained_command(cfg, ec, action).items():
                    self.states[a]["command"].append(float(v))
                if not failed[t]:
                    hist["reward"].append(float(rows[t, W_REWARD]))
            if not self.full[t]:
                continue
            values = {name: float(cols[name][t]) for name in names}
            target = {name: float(rows[t, W_TARGET + k]) for k, name in enumerate(names)}
            if ec.goal_enabled:   # goal status is evaluated against the pre-update target
                st = goal_status(ec, values, target if prev_target is None else prev_target)
                if hist["goal"] is None:
                    hist["goal"] = {k: [] for k in st}
                for k, v in st.items():
                    hist["goal"][k].append(v)
            for name in names:
                hist["target"][name].append(target[name])
                hist["error"][name].append(target_error(ec, name, values[name], target[name]))
            prev_target = target
        self.history = hist


class FlightRecorder(object):
    """Records the episodes of the envs `env_ids` of `vec` on the device: attach it BEFORE building a graphed rollout (a graph
    captured earlier replays without the recorder's launches).  An episode is recorded from its reset on: a tracked env shows
    nothing until the first vec.reset() that selects it after the attachment.  While attached, vec.reset / step / step_device each issue one
    more small launch; detach() restores the env's own launch sequence for every launch issued afterwards (it is refused while
    a graph captured with the recorder attached is alive: see detach)."""

    def __init__(self, vec, env_ids=(0,), max_steps=None):
        ids = [int(i) for i in np.atleast_1d(np.asarray(env_ids, dtype=np.int64))]
        if not 1 <= len(ids) <= nat.REC_MAX_TRACKED:
            raise ValueError("FlightRecorder tracks 1 .. {} envs, not {}".format(nat.REC_MAX_TRACKED, len(ids)))
        for i in ids:
            if not 0 <= i < vec.num_envs:
                raise ValueError("FlightRecorder: env id {} outside [0, {})".format(i, vec.num_envs))
        if getattr(vec, "_graph_mode", False) and getattr(vec, "_cap_token", None) is not None:
            raise RuntimeError("FlightRecorder: a launch sequence of this env has already been captured and would replay without "
                               "the recorder -- attach the recorder before building the (graphed) rollout")
        if getattr(vec, "_recorder", None) is not None:
            raise RuntimeError("FlightRecorder: the env already has a recorder attached (detach() it first)")
        self.vec, self.env_ids, self.K = vec, ids, len(ids)
        self.max_rows = int(max_steps or vec.cfg["steps_max"]) + 1
        m = vec._mem
        self._lib = vec._lib
        # (the backends have no 64-bit kind: the int64 ids travel as pairs of int32 words)
        self.ids = m.from_host(np.asarray(ids, dtype=np.int64).view(np.int32).reshape(self.K, 2), "i32")
        self.rows = m.zeros((2, self.K, self.max_rows, nat.REC_WORDS))
        self.hdr = m.zeros((self.K, nat.REC_HDR), "i32")
        vec._recorder = self

    def detach(self):
        """Takes the recorder's launches out of vec.reset / step / step_device.  Refused while a launch sequence captured with the
        recorder attached may still be replayed: its graph keeps the fwg_record nodes and their pointers into this recorder's
        buffers, which must stay alive (the env holds the recorder while it is attached).  Leave graph mode first
        (vec.set_graph_mode(False), dropping the captured graphs), then detach."""
        vec = self.vec
        if getattr(vec, "_recorder", None) is not self:
            return
        if getattr(vec, "_graph_mode", False) and getattr(vec, "_cap_token", None) is not None:
            raise RuntimeError("FlightRecorder.detach: a launch sequence captured with this recorder attached still holds its "
                               "launches and buffers -- drop the graph and leave graph mode (vec.set_graph_mode(False)) first")
        vec._recorder = None

    def slot_of(self, env_id):
        """Slot k of a tracked env id, or None."""
        return self.env_ids.index(int(env_id)) if int(env_id) in self.env_ids else None

    # -- the two launches (FixedWingVecEnv.reset / step_async / step_device call them) --------------------------------------
    def _on_reset(self, mask_t):
        v, m = self.vec, self.vec._mem
        nat.check(self._lib, self._lib.fwg_record_start(v._handle, m.ptr(self.ids), self.K, m.ptr(mask_t) if mask_t is not None else None,
                                                        m.ptr(self.rows), m.ptr(self.hdr), self.max_rows, m.stream()))

    def _on_step(self, actions, reward=None):
        """`reward`: where that step wrote its rewards (step_device's reward_out; default the env's own buffer)."""
        v, m = self.vec, self.vec._mem
        nat.check(self._lib, self._lib.fwg_record(v._handle, m.ptr(self.ids), self.K, m.ptr(actions), m.ptr(v._rew if reward is None else reward), m.ptr(v._done),
                                                  m.ptr(v._term), m.ptr(self.rows), m.ptr(self.hdr), self.max_rows, m.stream()))

    # -- reading ------------------------------------------------------------------------------------------------------------
    def header(self, k=0):
        """Host copy of slot k's header words (include/fwgym.h): one small read."""
        return np.array(self.vec._mem.to_host(self.hdr[k]), dtype=np.int32)

    def completed(self, k=0):
        """Number of episodes slot k's env has finished since the recorder was created."""
        return int(self.header(k)[6])

    def episode(self, k=0, which="last"):
        """The last completed episode of slot k (which="last") or the one in progress ("current"), decoded."""
        if which not in ("last", "current"):
            raise ValueError("which must be 'last' or 'current', not {!r}".format(which))
        h = self.header(k)
        flags, open_slab = int(h[0]), int(h[0]) & nat.REC_SLAB
        if which == "last":
            if h[6] == 0:
                raise RuntimeError("FlightRecorder: env {} has not completed an episode yet".format(self.env_ids[k]))
            slab, n, serial, over = open_slab ^ 1, int(h[2]), h[5], flags & nat.REC_OVERFLOW_DONE
        else:
            if not flags & nat.REC_OPEN:
                raise RuntimeError("FlightRecorder: env {} has no episode in progress".format(self.env_ids[k]))
            slab, n, serial, over = open_slab, int(h[1]), h[4], flags & nat.REC_OVERFLOW
        rows = np.array(self.vec._mem.to_host(self.rows[slab, k, :n]), dtype=np.float32)
        return Episode(self.vec, rows, int(h[3]), int(serial) & 0xFFFFFFFF, over, which == "last")

    def render(self, mode="plot", show=True, close=True, block=False, save_path=None, k=0, which="last"):
        """The reference's episode figure (FixedWingAircraft.render, fixed_wing.py:572-652) of a recorded episode."""
        ep = self.episode(k, which)
        return plot_episode(self.vec.cfg, self.vec.env_config, ep.states, ep.history, mode=mode, show=show, close=close, block=block,
                            save_path=save_path)[0]

    def save_history(self, path, states, save_targets=True, k=0, which="last"):
        """FixedWingAircraft.save_history (fixed_wing.py:654-672) of a recorded episode."""
        ep = self.episode(k, which)
        save_history_file(self.vec.cfg, self.vec.env_config, ep.states, ep.history, path, states, save_targets)
