"""Shared pieces of tests/test_eval_device.py (host emulation of the kernels) and tests/test_eval_device_gpu.py: the scripted
inputs and numpy restatement for the episode tracker (fwg_eval_advance), the open-loop inputs and float64 yardstick for the PID
head (fwg_pid_act), each run through a memory backend (emu.host_backend.HostBackend or the torch backend of vec_env)."""
import ctypes
import math

import numpy as np

from gym_fixed_wing import _native as nat
from oracle.pyfly_restated import PIDController

M = nat.N_METRICS
NULL = ctypes.c_void_p()
SENTINEL_ROWS = 64

# ---------------------------------------------------------------------------------------------------------------- tracker
TRACKER_N = (1, 63, 64, 65, 257)     # one lane, a wave minus one, a wave, a wave plus one, a workgroup plus one
TRACKER_T = 12


def tracker_inputs(N, T=TRACKER_T, seed=0):
    """Per step t: reward [N], done [N], term [N], the metrics block [M][N] as it stands after step t, the action batch [N][3] of
    step t.  Env e: e % 5 == 0 done at step 0 (and again later), e % 5 == 1 never done, e % 5 == 2 done at steps 3, 4 and 7, the
    others at random -- every done carries its own term code and its own metrics column.  NaN rewards and NaN action rows
    wherever the env has already ended (and in a few cells of running envs)."""
    rng = np.random.default_rng(1000 * N + seed)
    e = np.arange(N)
    done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    done[:, e % 5 == 1] = 0
    done[0, e % 5 == 0] = 1
    done[5, e % 5 == 0] = 1
    done[:, e % 5 == 2] = 0
    for t in (3, 4, 7):
        done[t, e % 5 == 2] = 1
    term = rng.integers(1, 40, size=(T, N)).astype(np.uint8)            # different at every step
    metrics = rng.normal(size=(T, M, N)).astype(np.float32)             # a fresh block at every step
    reward = rng.normal(size=(T, N)).astype(np.float32)
    actions = rng.uniform(-1, 1, size=(T, N, 3)).astype(np.float32)
    ended = np.cumsum(done, axis=0) > 0                                  # ended[t]: done at some step <= t
    reward[1:][ended[:-1]] = np.nan                                      # steps after the first end
    actions[1:][ended[:-1]] = np.nan
    reward[rng.random((T, N)) < 0.05] = np.nan                           # and a few of running envs: carried into the trace
    return reward, done, term, metrics, actions


def tracker_reference(reward, done, term, metrics, actions, final_init):
    """The twenty-line restatement of fwg_eval_advance over T steps + the closing call."""
    T, N = reward.shape
    active, length, termination = np.ones(N, bool), np.zeros(N, np.int32), np.zeros(N, np.uint8)
    final = np.full((M, N), final_init, np.float32)
    trace, gated = np.empty((T, N), np.float32), actions.copy()
    for t in range(T + 1):
        if t > 0:
            trace[t - 1] = np.where(active, reward[t - 1], np.nan)
            length[active] = t
            new = active & (done[t - 1] != 0)
            termination[new] = term[t - 1][new]
            final[:, new] = metrics[t - 1][:, new]
            active &= ~new
        if t < T:
            gated[t][~active] = 0.0
    return {"active": active.astype(np.uint8), "length": length, "termination": termination, "metrics_final": final,
            "trace": trace, "actions": gated}


def _padded(mem, a, kind, fill):
    """`a` followed by SENTINEL_ROWS * (row length) sentinel elements, as one backend buffer; returns (buffer, n)."""
    a = np.ascontiguousarray(a)
    row = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1
    tail = np.full(SENTINEL_ROWS * row, fill, a.dtype)
    return mem.from_host(np.concatenate([a.reshape(-1), tail]), kind), a.size


def run_tracker(lib, mem, N, final_init=-7.0):
    """Drives fwg_eval_advance through the scripted steps; returns (got, want, sentinels_ok)."""
    reward, done, term, metrics, actions = tracker_inputs(N)
    T = reward.shape[0]
    want = tracker_reference(reward, done, term, metrics, actions, final_init)
    sent_f, sent_u, sent_i = np.float32(12345.5), np.uint8(0xAB), np.int32(-77)
    active, n_a = _padded(mem, np.ones(N, np.uint8), "u8", sent_u)
    length, n_l = _padded(mem, np.zeros(N, np.int32), "i32", sent_i)
    termination, n_t = _padded(mem, np.zeros(N, np.uint8), "u8", sent_u)
    final, n_f = _padded(mem, np.full((M, N), final_init, np.float32), "f32", sent_f)
    trace, n_r = _padded(mem, np.full((T, N), sent_f, np.float32), "f32", sent_f)    # (needs no initialisation: every cell is written)
    acts = [_padded(mem, actions[t], "f32", sent_f) for t in range(T)]
    d_reward, d_done, d_term = mem.from_host(reward), mem.from_host(done, "u8"), mem.from_host(term, "u8")
    d_metrics = mem.from_host(metrics)
    for t in range(T + 1):
        prev = (NULL,) * 4 if t == 0 else (mem.ptr(d_reward[t - 1]), mem.ptr(d_done[t - 1]), mem.ptr(d_term[t - 1]), mem.ptr(d_metrics[t - 1]))
        nat.check(lib, lib.fwg_eval_advance(N, t, *prev, mem.ptr(active), mem.ptr(length), mem.ptr(termination), mem.ptr(final),
                                            mem.ptr(trace), T, mem.ptr(acts[t][0]) if t < T else NULL, mem.stream()))
    mem.sync()
    host = lambda b: np.array(mem.to_host(b))
    bufs = {"active": (host(active), n_a, sent_u), "length": (host(length), n_l, sent_i), "termination": (host(termination), n_t, sent_u),
            "metrics_final": (host(final), n_f, sent_f), "trace": (host(trace), n_r, sent_f)}
    got = {k: b[:n].reshape(want[k].shape) for k, (b, n, _) in bufs.items()}
    got["actions"] = np.stack([host(b)[:n].reshape(N, 3) for b, n in acts])
    sentinels = all((b[n:] == s).all() and b[n:].size > 0 for b, n, s in bufs.values()) and \
        all((host(b)[n:] == sent_f).all() for b, n in acts)
    return got, want, sentinels


def assert_tracker(got, want, sentinels):
    for k in ("active", "length", "termination", "metrics_final", "trace", "actions"):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)      # (NaN == NaN here: the positions must agree)
    assert sentinels, "a sentinel behind one of the buffers was overwritten"


def tracker_refusals(lib, mem):
    """Every refused argument set -> (status, message)."""
    N, T = 4, 3
    f = lambda shape, kind="f32": mem.zeros(shape, kind)
    rew, done, term, met = f((N,)), f((N,), "u8"), f((N,), "u8"), f((M, N))
    act, length, termn, final, trace, actions = f((N,), "u8"), f((N,), "i32"), f((N,), "u8"), f((M, N)), f((T, N)), f((N, 3))
    p = mem.ptr
    good = [N, 1, p(rew), p(done), p(term), p(met), p(act), p(length), p(termn), p(final), p(trace), T, p(actions), mem.stream()]
    assert lib.fwg_eval_advance(*good) == 0
    out = {}
    for name, idx, val in (("n_envs 0", 0, 0), ("n_envs negative", 0, -3), ("t negative", 1, -1), ("t beyond the trace", 1, T + 1),
                           ("null reward", 2, NULL), ("null done", 3, NULL), ("null term_code", 4, NULL), ("null metrics", 5, NULL),
                           ("null active", 6, NULL), ("null length", 7, NULL), ("null termination", 8, NULL), ("null metrics_final", 9, NULL)):
        args = list(good)
        args[idx] = val
        out[name] = (lib.fwg_eval_advance(*args), lib.fwg_last_error().decode())
    mem.sync()
    return out


# --------------------------------------------------------------------------------------------------------------- PID head
PID_N = (1, 65, 257)
PID_STEPS = 200
# all eight gains non-zero and none at its default (the default k_i_phi = 0 would hide its term)
PID_GAINS = dict(k_p_phi=1.3, k_i_phi=0.7, k_d_phi=0.4, k_p_theta=-3.1, k_i_theta=-0.9, k_d_theta=-0.25, k_p_V=0.35, k_i_V=0.2)
PID_OBS_STRIDE, PID_OBS_COLS = 11, (7, 2, 9, 0, 5, 3)       # roll, pitch, Va, omega_p, omega_q, omega_r: permuted, with gaps
PID_TARGET_STRIDE, PID_TARGET_COLS = 5, (3, 0, 2)           # roll, pitch, Va
PID_DT = 0.01
# Twice the worst error of the parent's BatchedPID (torch fp32 on the CPU) against float64 on these inputs, actions and
# integrators, over the three batch sizes: profiles/pid_head_errors.txt (tools/pid_head_errors.py writes it).  Twice, because
# contraction and sin / cos differ between torch and the kernel; never above 1e-3, so that one lost term (>= 1e-2) cannot pass.
PID_TORCH_WORST = 1.064e-06
PID_BOUND = min(2.0 * PID_TORCH_WORST, 1e-3)


def pid_inputs(N, steps=PID_STEPS, seed=0):
    """Open-loop inputs over the env's ranges as float32 [steps][N] arrays: roll / pitch / Va around a per-env target with a
    per-env offset of fixed sign (so that the integrals grow) plus noise, one row in eight with noise large enough to drive
    every output into either limit; body rates within +-2 rad/s."""
    rng = np.random.default_rng(77 * N + seed)
    sign = lambda: rng.choice([-1.0, 1.0], size=N)
    big = rng.random((steps, N)) < 0.125
    amp = lambda small, large: np.where(big, large, small) * rng.uniform(-1, 1, size=(steps, N))
    t_roll, t_pitch, t_va = rng.uniform(-0.5, 0.5, N), rng.uniform(-0.3, 0.3, N), rng.uniform(15, 25, N)
    roll = t_roll + sign() * rng.uniform(0.10, 0.15, N) + amp(0.15, 1.5)
    pitch = t_pitch + sign() * rng.uniform(0.03, 0.05, N) + amp(0.05, 0.6)
    va = t_va - rng.uniform(0.6, 1.0, N) + amp(0.6, 8.0)     # (below the target: the throttle works around 0.5, not at its lower limit)
    om = rng.uniform(-2, 2, size=(3, steps, N)) * np.where(big, 1.0, 0.25)
    f = lambda a: np.broadcast_to(a, (steps, N)).astype(np.float32)
    return {"roll": f(roll), "pitch": f(pitch), "Va": f(va), "omega_p": f(om[0]), "omega_q": f(om[1]), "omega_r": f(om[2]),
            "t_roll": f(t_roll), "t_pitch": f(t_pitch), "t_Va": f(t_va)}


def _oracle(gains):
    pid = PIDController(PID_DT)
    for k, v in gains.items():
        setattr(pid, k, v)
    return pid


def pid_float64(inp, gains=PID_GAINS):
    """oracle.pyfly_restated.PIDController in float64, driven open loop on all envs at once -> actions [steps][N][3],
    integrators [steps][3][N] (roll, pitch, Va; after each step)."""
    x = {k: v.astype(np.float64) for k, v in inp.items()}
    steps, N = x["roll"].shape
    pid = _oracle(gains)
    pid.int_va, pid.int_roll, pid.int_pitch = np.zeros(N), np.zeros(N), np.zeros(N)   # (three arrays: += works in place)
    acts, integ = np.empty((steps, N, 3)), np.empty((steps, 3, N))
    for t in range(steps):
        pid.set_reference(x["t_roll"][t], x["t_pitch"][t], x["t_Va"][t])
        acts[t] = pid.get_action(x["roll"][t], x["pitch"][t], x["Va"][t], [x["omega_p"][t], x["omega_q"][t], x["omega_r"][t]]).T
        integ[t] = np.stack([pid.int_roll, pid.int_pitch, pid.int_va])
    return acts, integ


def assert_pid_inputs_exercise_every_term(inp, gains=PID_GAINS):
    """The property of the INPUTS the comparison rests on, asserted on the float64 side: every output sits at each of its limits
    in some rows, and each of the eight terms moves its (clipped) output by >= 1e-2 in at least half of the rows."""
    acts, _ = pid_float64(inp, gains)
    lim = _oracle(gains)
    for col, lo, hi in ((0, lim.delta_e_min, lim.delta_e_max), (1, lim.delta_a_min, lim.delta_a_max), (2, 0.0, 1.0)):
        assert (acts[..., col] == lo).any() and (acts[..., col] == hi).any(), col
    out_of = {"k_p_phi": 1, "k_i_phi": 1, "k_d_phi": 1, "k_p_theta": 0, "k_i_theta": 0, "k_d_theta": 0, "k_p_V": 2, "k_i_V": 2}
    for k, col in out_of.items():
        # (the integrals of the comparison run stay those of the full controller: only the term's gain in the OUTPUT is dropped)
        without = _pid_float64_without(inp, gains, k)
        moved = np.abs(acts[..., col] - without[..., col]) >= 1e-2
        assert moved.mean() >= 0.5, (k, moved.mean())


def _pid_float64_without(inp, gains, dropped):
    x = {k: v.astype(np.float64) for k, v in inp.items()}
    steps, N = x["roll"].shape
    full, cut = _oracle(gains), _oracle(dict(gains, **{dropped: 0.0}))
    full.int_va, full.int_roll, full.int_pitch = np.zeros(N), np.zeros(N), np.zeros(N)
    acts = np.empty((steps, N, 3))
    for t in range(steps):
        args = (x["roll"][t], x["pitch"][t], x["Va"][t], [x["omega_p"][t], x["omega_q"][t], x["omega_r"][t]])
        for p in (full, cut):
            p.set_reference(x["t_roll"][t], x["t_pitch"][t], x["t_Va"][t])
        cut.int_va, cut.int_roll, cut.int_pitch = full.int_va.copy(), full.int_roll.copy(), full.int_pitch.copy()
        acts[t] = cut.get_action(*args).T
        full.get_action(*args)
    return acts


def pid_torch_fp32(inp, gains=PID_GAINS):
    """The parent's BatchedPID in torch fp32 on the CPU on the same inputs (what the asserted bound is measured on)."""
    import torch
    from gym_fixed_wing.pid import BatchedPID
    steps, N = inp["roll"].shape
    pid = BatchedPID(N, dt=PID_DT, device="cpu")
    for k, v in gains.items():
        setattr(pid, k, v)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    acts, integ = np.empty((steps, N, 3), np.float32), np.empty((steps, 3, N), np.float32)
    for t in range(steps):
        pid.set_reference(T(inp["t_roll"][t]), T(inp["t_pitch"][t]), T(inp["t_Va"][t]))
        om = torch.stack([T(inp["omega_p"][t]), T(inp["omega_q"][t]), T(inp["omega_r"][t])], dim=1)
        acts[t] = pid.get_action(T(inp["roll"][t]), T(inp["pitch"][t]), T(inp["Va"][t]), om).numpy()
        integ[t] = torch.stack([pid.int_roll, pid.int_pitch, pid.int_va]).numpy()
    return acts, integ


def pid_errors(acts, integ, inp, gains=PID_GAINS):
    """Worst absolute error of the actions (per output) and of the integrators against float64."""
    want_a, want_i = pid_float64(inp, gains)
    ea = np.abs(acts.astype(np.float64) - want_a).max(axis=(0, 1))
    ei = np.abs(integ.astype(np.float64) - want_i).max(axis=(0, 2))
    return {"elevator": ea[0], "aileron": ea[1], "throttle": ea[2], "int_roll": ei[0], "int_pitch": ei[1], "int_Va": ei[2]}


def pid_gains_struct(gains=PID_GAINS):
    from gym_fixed_wing.pid import default_gains
    g = default_gains(PID_DT)
    g.update(gains)
    return nat.PidGains(**{k: float(v) for k, v in g.items()})


def run_pid(lib, mem, N, gains=PID_GAINS):
    """fwg_pid_act open loop over pid_inputs(N): rows wider than the columns used (the rest NaN), permuted columns.  Returns
    actions [steps][N][3], integrators [steps][3][N] (host) and the inputs."""
    inp = pid_inputs(N)
    steps = inp["roll"].shape[0]
    obs = np.full((steps, N, PID_OBS_STRIDE), np.nan, np.float32)
    for c, k in zip(PID_OBS_COLS, ("roll", "pitch", "Va", "omega_p", "omega_q", "omega_r")):
        obs[:, :, c] = inp[k]
    tgt = np.full((steps, N, PID_TARGET_STRIDE), np.nan, np.float32)
    for c, k in zip(PID_TARGET_COLS, ("t_roll", "t_pitch", "t_Va")):
        tgt[:, :, c] = inp[k]
    d_obs, d_tgt = mem.from_host(obs), mem.from_host(tgt)
    d_act, d_int, d_int_log = mem.zeros((steps, N, 3)), mem.zeros((3, N)), mem.zeros((steps, 3, N))
    oc, tc, g = (ctypes.c_int32 * 6)(*PID_OBS_COLS), (ctypes.c_int32 * 3)(*PID_TARGET_COLS), pid_gains_struct(gains)
    for t in range(steps):
        nat.check(lib, lib.fwg_pid_act(N, mem.ptr(d_obs[t]), PID_OBS_STRIDE, oc, mem.ptr(d_tgt[t]), PID_TARGET_STRIDE, tc, g,
                                       mem.ptr(d_int), mem.ptr(d_act[t]), mem.stream()))
        d_int_log[t] = d_int      # (stream-ordered copy: no host read inside the loop)
    mem.sync()
    return np.array(mem.to_host(d_act)), np.array(mem.to_host(d_int_log)), inp


def pid_refusals(lib, mem):
    N = 4
    obs, tgt, integ, act = mem.zeros((N, 6)), mem.zeros((N, 3)), mem.zeros((3, N)), mem.zeros((N, 3))
    oc, tc, g, p = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5), (ctypes.c_int32 * 3)(0, 1, 2), pid_gains_struct(), mem.ptr
    good = [N, p(obs), 6, oc, p(tgt), 3, tc, g, p(integ), p(act), mem.stream()]
    assert lib.fwg_pid_act(*good) == 0
    out = {}
    for name, idx, val in (("n_envs 0", 0, 0), ("n_envs negative", 0, -1), ("null obs", 1, NULL), ("obs column at the stride", 2, 5),
                           ("null obs columns", 3, None), ("null target", 4, NULL), ("target column at the stride", 5, 2),
                           ("null target columns", 6, None), ("null integrators", 8, NULL), ("null actions", 9, NULL),
                           ("negative obs column", 3, (ctypes.c_int32 * 6)(0, -1, 2, 3, 4, 5))):
        args = list(good)
        args[idx] = val
        out[name] = (lib.fwg_pid_act(*args), lib.fwg_last_error().decode())
    mem.sync()
    return out


def ceil_div(a, b):
    return int(math.ceil(a / float(b)))
