"""Shared pieces of tests/test_monitor.py (host emulation of the kernels) and tests/test_monitor_gpu.py: the device training
monitor (include/fwgym.h "Training monitor": fwg_monitor_fold, fwg_monitor_take; gym_fixed_wing.monitor).  Every body runs through
either memory backend: `kw` are the FixedWingVecEnv keywords that select it (emu.host_backend.HostBackend + the emulation
library, or device=0).  All sums of the kernel are integers, so every comparison here is bit for bit."""
import csv
import ctypes
import types

import numpy as np
import torch

import configs
from gym_fixed_wing import _native as nat
from gym_fixed_wing import monitor as mon
from gym_fixed_wing.actor import DeviceActor
from gym_fixed_wing.monitor import EpisodeMonitor, ProgressLog
from gym_fixed_wing.ppo import PPO
from gym_fixed_wing.recorder import FlightRecorder
from gym_fixed_wing.rollout import FusedRollout, MlpPolicy
from gym_fixed_wing.vec_env import FixedWingVecEnv

NULL = ctypes.c_void_p()
SCALE = np.float32(1048576.0)
BAD = 0x80000000
SEG, SPAN = 32, 128                     # the kernel's split: FWG_MON_L steps per wave, four waves per span
CONTRACT_N = (1, 63, 64, 130, 4096)     # 130: two full waves and a tail of 2
CONTRACT_T = (1, 7, 127, 128, 129, 300)  # 300: more than two spans; 127 / 129: span -+ 1
PATTERNS = ("never", "every", "first", "last", "before_boundary", "on_boundary", "both_sides", "bernoulli_05", "bernoulli_5")


def backend(kw):
    """(library, memory backend) of a test's `kw`."""
    lib = nat.load_library(kw.get("_lib_path"))
    if kw.get("_backend") is not None:
        return lib, kw["_backend"]
    from gym_fixed_wing.vec_env import _TorchBackend
    return lib, _TorchBackend(kw["device"])


def bare_monitor(kw, n):
    """An EpisodeMonitor over `n` envs with no env behind it (fold / take need the library and the memory backend only)."""
    lib, mem = backend(kw)
    return EpisodeMonitor(types.SimpleNamespace(_lib=lib, _mem=mem, num_envs=n, _monitor=None))


# ----------------------------------------------------------------------------------------------------- the numpy restatement
class RefMonitor(object):
    """include/fwgym.h "Training monitor", restated: carries ep_q int64 [N] / ep_len uint32 [N] and the eight aggregates as
    Python integers (None for a minimum / maximum of nothing)."""

    def __init__(self, n):
        self.ep_q, self.ep_len = np.zeros(n, np.int64), np.zeros(n, np.uint32)
        self.clear()

    def clear(self):
        self.agg = {"episodes": 0, "nonfinite": 0, "sum_q": 0, "sum_len": 0, "min_q": None, "max_q": None, "min_len": None, "max_len": None}

    def fold(self, rew, done):
        rew = np.asarray(rew, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            bad = ~(np.abs(rew) <= SCALE)
            q = np.rint(np.where(bad, np.float32(0), rew) * SCALE).astype(np.int64)   # float32 product, ties to even
        a = self.agg
        for t in range(rew.shape[0]):
            self.ep_q += np.where(bad[t], 0, q[t])
            self.ep_len |= np.where(bad[t], np.uint32(BAD), np.uint32(0))
            self.ep_len += np.uint32(1)
            d = np.asarray(done[t]) != 0
            flagged = d & ((self.ep_len & np.uint32(BAD)) != 0)
            ok = d & ~flagged
            a["nonfinite"] += int(flagged.sum())
            if ok.any():
                qs, ls = [int(v) for v in self.ep_q[ok]], [int(v) for v in self.ep_len[ok]]
                a["episodes"] += len(qs)
                a["sum_q"] += sum(qs)
                a["sum_len"] += sum(ls)
                for key, vals, pick in (("min_q", qs, min), ("max_q", qs, max), ("min_len", ls, min), ("max_len", ls, max)):
                    a[key] = pick(vals) if a[key] is None else pick(a[key], pick(vals))
            self.ep_q[d] = 0
            self.ep_len[d] = 0

    def take(self):
        """The 8 doubles of fwg_monitor_take; clears the aggregates."""
        a, inf = self.agg, float("inf")
        some = a["episodes"] > 0
        out = np.array([a["episodes"], a["nonfinite"], float(a["sum_q"]) / 2.0 ** 20, a["sum_len"],
                        float(a["min_q"]) / 2.0 ** 20 if some else inf, float(a["max_q"]) / 2.0 ** 20 if some else -inf,
                        a["min_len"] if some else inf, a["max_len"] if some else -inf], np.float64)
        self.clear()
        return out


def take_doubles(m):
    """fwg_monitor_take through an EpisodeMonitor -> the 8 doubles on the host."""
    return np.ascontiguousarray(m.vec._mem.to_host(m.take_device())).view(np.float64).copy()


def assert_same(m, ref, what):
    """Both carries now, then one take of each: all 8 doubles, bit for bit."""
    q, length = m.carries()
    np.testing.assert_array_equal(q, ref.ep_q, err_msg="{}: ep_q carry".format(what))
    np.testing.assert_array_equal(length.view(np.uint32), ref.ep_len, err_msg="{}: ep_len carry".format(what))
    got, want = take_doubles(m), ref.take()
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64), err_msg="{}: take {} != {}".format(what, got, want))
    return got


# ------------------------------------------------------------------------------------------------------- synthetic rollouts
def done_pattern(name, T, rng):
    t = np.arange(T)
    if name == "never":
        return np.zeros(T, bool)
    if name == "every":
        return np.ones(T, bool)
    if name == "first":
        return t == 0
    if name == "last":
        return t == T - 1
    if name == "before_boundary":            # s0 - 1 of every segment (and s1 - 1 of the one before it)
        return t % SEG == SEG - 1
    if name == "on_boundary":                # s0 of every segment
        return t % SEG == 0
    if name == "both_sides":
        return (t % SEG == SEG - 1) | (t % SEG == 0)
    return rng.random(T) < (0.05 if name == "bernoulli_05" else 0.5)


def synthetic(T, N, shift=0, seed=0, bad_rate=0.01):
    """raw_rewards float32 [T][N] and dones uint8 [T][N]: env e follows done pattern (e + shift) mod 9; rewards of both signs,
    a tenth of them exact ties at (k + 0.5) 2^-20 (the rounding mode), the bound 2^20 itself (good) and, at `bad_rate`, a NaN, an
    inf or +-2e6 (bad), wherever they fall relative to the dones."""
    rng = np.random.default_rng([seed, T, N, shift])
    rew = (rng.standard_normal((T, N)) * 3.0).astype(np.float32)
    ties = rng.random((T, N)) < 0.1
    k = rng.integers(-4000000, 4000000, size=(T, N))
    rew[ties] = ((k[ties] + 0.5) * 2.0 ** -20).astype(np.float32)       # exact: |k + 0.5| < 2^23
    edge = rng.random((T, N)) < 0.01
    rew[edge] = np.where(rng.random(int(edge.sum())) < 0.5, SCALE, -SCALE)
    hit = rng.random((T, N)) < bad_rate
    rew[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 2e6, -2e6, np.nextafter(SCALE, np.float32(np.inf))], np.float32), int(hit.sum()))
    done = np.stack([done_pattern(PATTERNS[(e + shift) % len(PATTERNS)], T, rng) for e in range(N)], axis=1)
    return rew, done.astype(np.uint8)


def fold(m, rew, done):
    mem = m.vec._mem
    m.fold(mem.from_host(rew), mem.from_host(done, "u8"))


def run_contract(kw, N, T):
    """One (N, T) cell: every done pattern reaches env 0 (shifts) when N is smaller than the pattern list; two folds with a
    take after each (the second starts from the first one's carries)."""
    for shift in (range(len(PATTERNS)) if N < len(PATTERNS) else (0,)):
        m, ref = bare_monitor(kw, N), RefMonitor(N)
        for part in range(2):
            rew, done = synthetic(T, N, shift, seed=part)
            fold(m, rew, done)
            ref.fold(rew, done)
            assert_same(m, ref, "N {} T {} shift {} fold {}".format(N, T, shift, part))


def bad_reward_cases(kw):
    """A NaN, an inf and 2e6 placed before, on and after a done: T = 9, a done at t = 4 and one at t = 8; env 3 v + p has value v
    at t = 3 (before), 4 (on) or 5 (after).  The flag hits exactly one episode and is gone after it.  Returns the 8 doubles."""
    values = [np.nan, np.inf, 2e6]
    T, N = 9, 9
    rew = np.full((T, N), 0.25, np.float32)
    done = np.zeros((T, N), np.uint8)
    done[4], done[8] = 1, 1
    for v, value in enumerate(values):
        for p, t in enumerate((3, 4, 5)):
            rew[t, 3 * v + p] = value
    m, ref = bare_monitor(kw, N), RefMonitor(N)
    fold(m, rew, done)
    ref.fold(rew, done)
    q, length = m.carries()
    assert not q.any() and not length.any()                    # every env ended at t = 8: nothing open, no flag left
    return assert_same(m, ref, "bad rewards")


def carry_cases(kw):
    """Three folds with an episode that spans all three; two folds before one take; a take with no episode; a second take."""
    N, T = 70, 40
    rng = np.random.default_rng(3)
    m, ref = bare_monitor(kw, N), RefMonitor(N)
    out = {}
    out["empty"] = assert_same(m, ref, "take before any fold")
    parts = []
    for part in range(3):
        rew = (rng.standard_normal((T, N)) * 2.0).astype(np.float32)
        done = (rng.random((T, N)) < 0.03).astype(np.uint8)
        done[:, :5] = 0                                          # envs 0..4: one episode through all three folds ...
        if part == 2:
            done[T - 3, :5] = 1                                  # ... that ends in the third
        parts.append((rew, done))
    fold(m, *parts[0]); ref.fold(*parts[0])
    fold(m, *parts[1]); ref.fold(*parts[1])                      # two folds, one take
    out["two_folds"] = assert_same(m, ref, "two folds before one take")
    fold(m, *parts[2]); ref.fold(*parts[2])
    got = assert_same(m, ref, "third fold")
    assert got[7] >= 2 * T + T - 2                               # the episode through all three folds
    out["again"] = assert_same(m, ref, "a second take right after")
    return out


def sharding_case(kw, N=130, n1=37, T=140):
    rew, done = synthetic(T, N, seed=9)
    whole, a, b = bare_monitor(kw, N), bare_monitor(kw, n1), bare_monitor(kw, N - n1)
    fold(whole, rew, done)
    fold(a, np.ascontiguousarray(rew[:, :n1]), np.ascontiguousarray(done[:, :n1]))
    fold(b, np.ascontiguousarray(rew[:, n1:]), np.ascontiguousarray(done[:, n1:]))
    qa, la = a.carries()
    qb, lb = b.carries()
    qw, lw = whole.carries()
    np.testing.assert_array_equal(np.concatenate([qa, qb]), qw)
    np.testing.assert_array_equal(np.concatenate([la, lb]), lw)
    parts = mon.combine([take_doubles(a), take_doubles(b)])
    total = take_doubles(whole)
    np.testing.assert_array_equal(parts.view(np.int64), total.view(np.int64))
    assert total[0] > 100 and total[1] > 0
    return total


def refusals(kw):
    """name -> (status, message) of calls that must launch nothing."""
    lib, mem = backend(kw)
    N, T = 8, 4
    rew, done = mem.zeros((T, N)), mem.zeros((T, N), "u8")
    q, length, scratch, out = mem.zeros((N, 2), "i32"), mem.zeros((N,), "i32"), mem.zeros((16,), "i32"), mem.zeros((16,), "i32")
    p = mem.ptr
    full = [T, N, p(rew), p(done), p(q), p(length), p(scratch), mem.stream()]
    calls = {"n_steps 0": lambda: lib.fwg_monitor_fold(*([0] + full[1:])), "n_steps -1": lambda: lib.fwg_monitor_fold(*([-1] + full[1:])),
             "n_envs 0": lambda: lib.fwg_monitor_fold(*([T, 0] + full[2:])), "n_envs -3": lambda: lib.fwg_monitor_fold(*([T, -3] + full[2:])),
             "take n_envs 0": lambda: lib.fwg_monitor_take(0, p(scratch), p(out), mem.stream()),
             "take null scratch": lambda: lib.fwg_monitor_take(N, NULL, p(out), mem.stream()),
             "take null out": lambda: lib.fwg_monitor_take(N, p(scratch), NULL, mem.stream())}
    for i, name in ((2, "raw_rewards"), (3, "dones"), (4, "ep_q_io"), (5, "ep_len_io"), (6, "scratch")):
        args = list(full)
        args[i] = NULL
        calls["null " + name] = (lambda a: lambda: lib.fwg_monitor_fold(*a))(args)
    res = {}
    for name, call in calls.items():
        status = call()
        res[name] = (status, lib.fwg_last_error().decode())
    mem.sync()
    for t in (q, length, scratch, out):
        assert not np.asarray(mem.to_host(t)).any()                 # nothing was launched
    assert lib.fwg_monitor_scratch_bytes(0) == 0 and lib.fwg_monitor_scratch_bytes(-5) == 0
    assert lib.fwg_monitor_scratch_bytes(1) == 64 and lib.fwg_monitor_scratch_bytes(64) == 64 and lib.fwg_monitor_scratch_bytes(65) == 128
    return res


# ------------------------------------------------------------------------------------------------------- through the layers
ENVS, STEPS_MAX, N_STEPS = 70, 10, 6


def small_env(kw, n=ENVS, steps_max=STEPS_MAX, seed=2):
    vec = FixedWingVecEnv(configs.reference_like("examples"), num_envs=n, config_kw={"steps_max": steps_max}, seed=seed, **kw)
    vec.reset()
    return vec


def small_head(vec):
    torch.manual_seed(0)
    policy = MlpPolicy(vec.obs_dim)
    with torch.no_grad():
        policy.log_std.copy_(torch.tensor([-1.0, -0.7, -1.2]))
    actor = DeviceActor.for_env(vec, seed=5)
    actor.load_policy(policy)
    return actor


def host(vec, t):
    return np.array(vec._mem.to_host(t))


def raw_rewards_rollout(kw, rollouts=4):
    """FusedRollout(raw_rewards=True), eager with a tap, beside a twin without the flag: every row of buf["raw_rewards"] is the
    reward the tap saw, every other buffer equals the twin's, and the monitor's take equals the numpy fold of the buffers."""
    seen = {"raw": [], "twin": []}
    runs = {}
    for name in ("raw", "twin"):
        vec = small_env(kw)
        actor = small_head(vec)
        tap = (lambda rows: lambda t, o, r, d: rows.append(host(vec, r).copy()))(seen[name])
        runs[name] = (vec, actor, FusedRollout(vec, actor, N_STEPS, tap=tap, raw_rewards=name == "raw"))
    vec, _, ro = runs["raw"]
    assert not ro.fused and "raw_rewards" in ro.buf and "raw_rewards" not in runs["twin"][2].buf
    m, ref = EpisodeMonitor(vec), RefMonitor(ENVS)
    episodes = 0
    launches = {name: 0 for name in runs}
    real_check = nat.check
    for r in range(rollouts):
        seen["raw"].clear(), seen["twin"].clear()
        bufs = {}
        for name, (v, _, ro_) in runs.items():
            def counting(lib, status, name=name):                # every launch of the package goes through nat.check
                launches[name] += 1
                return real_check(lib, status)
            nat.check = counting
            try:
                bufs[name] = {k: host(v, b) for k, b in ro_.run().items()}
            finally:
                nat.check = real_check
        raw = bufs["raw"].pop("raw_rewards")
        np.testing.assert_array_equal(raw.view(np.int32), np.stack(seen["raw"]).view(np.int32), err_msg="rollout {}: raw rows vs tap".format(r))
        np.testing.assert_array_equal(raw.view(np.int32), np.stack(seen["twin"]).view(np.int32), err_msg="rollout {}: raw rows vs twin".format(r))
        for k in bufs["twin"]:
            np.testing.assert_array_equal(bufs["raw"][k].view(np.uint8), bufs["twin"][k].view(np.uint8), err_msg="rollout {} buffer {}".format(r, k))
        m.fold(ro.buf["raw_rewards"], ro.buf["dones"])
        ref.fold(raw, bufs["raw"]["dones"])
        episodes += int(assert_same(m, ref, "rollout {}".format(r))[0])
    assert not host(vec, vec._rew).any()                          # the env's own reward buffer was never written
    assert launches["raw"] == launches["twin"] > 2 * N_STEPS * rollouts   # no extra launch with the flag
    assert episodes >= ENVS * (rollouts * N_STEPS // STEPS_MAX)
    for v, actor, _ in runs.values():
        actor.close()
        v.close()


def one_launch_step_refuses_raw_rewards(kw):
    vec = small_env(kw)
    actor = small_head(vec)
    try:
        FusedRollout(vec, actor, 4, fused=True, raw_rewards=True)
        raised = None
    except ValueError as e:
        raised = str(e)
    assert raised is not None and "two-launch" in raised
    assert not FusedRollout(vec, actor, 4, fused="auto", raw_rewards=True).fused
    assert not FusedRollout(vec, actor, 4, raw_rewards=True).fused
    bad = vec._mem.zeros((vec.num_envs + 1,))
    try:
        vec.step_device(vec._mem.zeros((vec.num_envs, 3)), reward_out=bad)
        raised = None
    except ValueError as e:
        raised = str(e)
    assert raised is not None and "reward_out" in raised
    actor.close()
    vec.close()


def recorder_and_monitor_together(kw, rollouts=4):
    """The recorder is handed the rollout's reward row: its headers and rows equal those of a run with the recorder alone."""
    state = {}
    for name in ("both", "alone"):
        vec = FixedWingVecEnv(configs.reference_like("examples"), num_envs=ENVS, config_kw={"steps_max": STEPS_MAX}, seed=2, **kw)
        rec = FlightRecorder(vec, env_ids=(0, 64, ENVS - 1))
        vec.reset()
        actor = small_head(vec)
        ro = FusedRollout(vec, actor, N_STEPS, raw_rewards=name == "both")
        for _ in range(rollouts):
            ro.run()
        state[name] = (host(vec, rec.hdr), host(vec, rec.rows).view(np.int32))
        assert state[name][0][:, 6].min() >= 2
        rewards = [rec.episode(k, "last").history["reward"] for k in range(3)]
        assert all(len(r) >= 1 and np.isfinite(r).all() and np.any(np.asarray(r) != 0) for r in rewards)
        actor.close()
        vec.close()
    np.testing.assert_array_equal(state["both"][0], state["alone"][0])
    np.testing.assert_array_equal(state["both"][1], state["alone"][1])


def window_pools_takes(kw):
    """4 envs: every take holds 4 episodes, so window(100) pools the last 25 takes (and window(4) the last one)."""
    m = bare_monitor(kw, 4)
    assert m.window(100) == {"episodes": 0, "ep_rew_mean": None, "ep_len_mean": None}
    sums = []
    for i in range(30):
        T = 3 + i % 4
        rew = np.full((T, 4), 0.5 * (i + 1), np.float32)
        done = np.zeros((T, 4), np.uint8)
        done[T - 1] = 1
        fold(m, rew, done)
        res = m.take()
        assert res["episodes"] == 4 and res["ep_len_mean"] == T and res["ep_rew_mean"] == 0.5 * (i + 1) * T
        assert res["ep_rew_min"] == res["ep_rew_max"] == res["ep_rew_mean"] and res["ep_len_min"] == res["ep_len_max"] == T
        sums.append((4 * 0.5 * (i + 1) * T, 4 * T))
    w = m.window(100)
    assert w["episodes"] == 100
    assert w["ep_rew_mean"] == sum(s for s, _ in sums[-25:]) / 100 and w["ep_len_mean"] == sum(n for _, n in sums[-25:]) / 100
    assert m.window(4)["ep_len_mean"] == sums[-1][1] / 4 and m.window(5)["episodes"] == 8
    assert m.take() == {k: (0 if k in ("episodes", "nonfinite") else None) for k in mon.TAKE_KEYS}


def reset_zeroes_the_carries(kw):
    vec = small_env(kw, n=6)
    m = EpisodeMonitor(vec)
    try:
        EpisodeMonitor(vec)
        raised = False
    except RuntimeError:
        raised = True
    assert raised
    rew, done = np.full((3, 6), 1.5, np.float32), np.zeros((3, 6), np.uint8)
    rew[1, 2] = np.nan
    fold(m, rew, done)
    q, length = m.carries()
    assert (np.delete(q, 2) == 3 * 1.5 * 2 ** 20).all() and (np.delete(length, 2) == 3).all() and length.view(np.uint32)[2] == BAD | 3
    vec.reset(indices=[1, 2])
    q, length = m.carries()
    assert list(q != 0) == [True, False, False, True, True, True] and list(length != 0) == [True, False, False, True, True, True]
    vec.reset()
    q, length = m.carries()
    assert not q.any() and not length.any()
    assert take_doubles(m)[0] == 0                                # an abandoned episode is never emitted
    m.detach()
    assert vec._monitor is None
    vec.close()


NEW_KEYS = set(mon.TAKE_KEYS) - {"episodes"} | {"monitor_episodes", "ep_rew_mean_100", "ep_len_mean_100", "ep_info"}


def ppo_with_and_without_the_monitor(kw, log_dir):
    """PPO(monitor=True) beside PPO(monitor=False), two updates at 4 envs with steps_max 5 (every episode times out): the
    episode length, the five measures, the untouched `info` of the plain run, equal weights, and the CSV of ProgressLog."""
    steps_max, n, n_steps = 5, 4, 10
    runs = {}
    printed = []
    for monitor in (True, False):
        vec = small_env(kw, n=n, steps_max=steps_max, seed=3)
        ppo = PPO(vec, seed=0, n_steps=n_steps, nminibatches=2, noptepochs=2, monitor=monitor)
        ppo.learn(2 * n_steps * n, log=ProgressLog(log_dir, log_interval=1, out=printed.append) if monitor else None)
        runs[monitor] = (vec, ppo)
    log = ProgressLog(log_dir)            # (the path only: nothing is written before the first call)
    (vec, ppo), (_, plain) = runs[True], runs[False]
    assert len(ppo.history) == len(plain.history) == 2
    assert "raw_rewards" in ppo.rollout.buf and "raw_rewards" not in plain.rollout.buf and plain.monitor is None
    for info, base in zip(ppo.history, plain.history):
        assert not NEW_KEYS & set(base) and NEW_KEYS <= set(info)
        assert {k: v for k, v in info.items() if k not in NEW_KEYS} == base      # (same weights, same episodes: same numbers)
        assert info["episodes"] == info["monitor_episodes"] == n * (n_steps // steps_max) and info["nonfinite"] == 0
        assert info["ep_len_mean"] == steps_max and info["ep_len_min"] == info["ep_len_max"] == steps_max
        assert info["ep_rew_min"] <= info["ep_rew_mean"] <= info["ep_rew_max"] and info["ep_rew_min"] < info["ep_rew_max"]
        assert set(mon.MEASURES) <= set(info["ep_info"]) and info["ep_info"]["episodes"] == info["episodes"]
        names = list(vec.target_names)
        for measure in mon.MEASURES:
            want = ["all"] if measure == "control_variation" else names + (["all"] if measure in ("success", "success_time_frac") else [])
            assert list(info["ep_info"][measure]) == want and all(np.isfinite(v) for v in info["ep_info"][measure].values())
    last = ppo.history[-1]
    total = sum(i["monitor_episodes"] for i in ppo.history)
    assert last["ep_len_mean_100"] == steps_max
    assert last["ep_rew_mean_100"] == sum(i["ep_rew_mean"] * i["monitor_episodes"] for i in ppo.history) / total
    for (ka, a), (kb, b) in zip(ppo.policy.state_dict().items(), plain.policy.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    # the log file: a header and one row per update, every cell the flattened info's value
    with open(log.path, newline="") as f:
        rows = list(csv.reader(f))
    assert len(rows) == 3 and rows[0] == list(mon.flatten(ppo.history[0]))
    assert {"ep_rew_mean", "ep_len_mean", "ep_info/end_error/roll", "ep_info/success_time_frac/all", "timesteps"} <= set(rows[0])
    for cells, info in zip(rows[1:], ppo.history):
        flat = mon.flatten(info)
        for key, cell in zip(rows[0], cells):
            want = flat.get(key)
            assert cell == ("" if want is None else str(want)), key
            if isinstance(want, float):
                assert float(cell) == want
    assert len(printed) == 2 and printed[0].startswith("\nsuccess:\n\troll      ") and "\ntotal_error:\n\t" in printed[0]
    assert printed[1] == ProgressLog.block(last["ep_info"])
    for v, p in runs.values():
        p.actor.close()
        v.close()
