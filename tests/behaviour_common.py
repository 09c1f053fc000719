"""Shared pieces of tests/test_behaviour.py: the behaviour head and the hindsight collector (include/fwgym.h "Behaviour head",
gym_fixed_wing/behaviour.py, csrc/fwgym_behaviour.h) on the host emulation of the kernels and on the GPU.  Every body takes
(lib, device): the emulation library with "cpu", or the HIP library with cuda:0.

Weights: offpolicy_common.make_nets (tanh neither linear nor saturated).  Observations and goals: seeded normal.  Every output
buffer has one more row than the batch, filled with NaN (255 for flags), which must still be there afterwards.

Bounds.
  ACTION_TOL   the forward pass against GoalActor in float64: measured maximum absolute action error over all shapes, 1.253e-5 on the
               emulation and 1.235e-5 on the GPU (profiles/behaviour_head_errors.txt); asserted at twice the larger, rounded up to one
               significant digit: 3e-5.  The expectation was at or below 1e-5; the measurement is a quarter above it, and ppo_tanh is
               NOT why: its restatement in fp32 on the exact pre-activations is within 1.4e-7 of tanh, and torch's own fp32 forward
               within 2.5e-7 of float64 on the same inputs.  The error is ddpg_forward's split-operand products: each fp32 operand
               enters the matrix cores as bf16 hi + bf16 lo, 16 mantissa bits, and lo x lo is dropped, so a product carries a relative
               error of ~2^-16 = 1.5e-5 of its magnitude, not fp32's 6e-8.  make_nets scales both hidden layers by 4 (its rejection
               rule needs it), which puts |pre-activation 2| at up to ~30; 2^-17 x the ~64 terms behind such a unit is ~1e-4 absolute
               in the hidden layer, and the output layer (weights scaled by 3/16, tanh slope <= 1) brings ~1e-5 of it to the action.
               The same products, at the same precision, are what DDPG(update="hip") differentiates (tests/test_offpolicy_contract.py
               holds its gradients to 1e-4 relative), so the head acts on the network the learner trains.
  UNIFORM_TOL  1e-6: 2 u - 1 is two fp32 roundings on values in [-1, 1].
  the Gaussian branch: ACTION_TOL + sigma x (2 x the error of the device box_muller), that error measured in the test itself on the
               EXISTING policy head's noise (fwg_actor_act with zero weights and log_std 0: its action is its noise) against
               oracle.physics.box_muller over the same number of draws."""
import copy
import ctypes

import numpy as np
import torch

import offpolicy_common as oc
from gym_fixed_wing import _native as nat
from gym_fixed_wing.behaviour import BehaviourHead, HindsightCollector, eps_scaled
from gym_fixed_wing.offpolicy import DDPG
from oracle import physics as oph

SHAPES = [(11, 3, 3), (13, 3, 3), (14, 3, 3), (57, 3, 4), (60, 1, 1)]
BATCHES = [1, 63, 64, 65, 130]
ACTION_TOL = 3e-5
UNIFORM_TOL = 1e-6
STREAM = 12   # FWG_STREAM_BEHAVIOUR


def fenced(device, n, cols=None, kind=torch.float32):
    """(full, view): n rows for the kernel and one guard row behind them."""
    shape = (n + 1,) if cols is None else (n + 1, cols)
    full = torch.full(shape, 255 if kind == torch.uint8 else float("nan"), dtype=kind, device=device)
    return full, full[:n]


def fence_holds(full):
    last = full[-1].cpu()
    return bool((last == 255).all()) if full.dtype == torch.uint8 else bool(torch.isnan(last).all())


def make_agent(lib, device, shape, seed, update="hip"):
    """A DDPG whose actor carries make_nets' weights (the float64 reference is a copy of the same module)."""
    D, G, A = shape
    nets = oc.make_nets(D, G, A, 1, seed)
    agent = DDPG(D, G, A, update=update, device=device, seed=seed, _lib=lib)
    agent.actor.load_state_dict(nets[0].state_dict())   # (update="hip": copied into the views of the flat vector)
    return agent, copy.deepcopy(nets[0]).double()


def inputs(shape, n, seed, device):
    D, G, _ = shape
    gen = torch.Generator().manual_seed(seed)
    obs = (torch.randn(n, D, generator=gen, dtype=torch.float64) * 1.5).float()
    rows = torch.zeros(n, 4)
    rows[:, :G] = torch.randn(n, G, generator=gen, dtype=torch.float64).float()
    return obs.to(device).contiguous(), rows.to(device).contiguous()


def pi64(actor64, obs, rows):
    G = actor64.goal_dim
    with torch.no_grad():
        return actor64(obs.cpu().double(), rows.cpu().double()[:, :G]).numpy()


def bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().contiguous().view(torch.uint8 if t.dtype == torch.uint8 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
def forward_error(lib, device, shape, n, seed):
    """Maximum absolute error of the deterministic actions against GoalActor in float64; rows past n untouched."""
    agent, ref = make_agent(lib, device, shape, seed)
    head = BehaviourHead(agent, n, _lib=lib)
    obs, rows = inputs(shape, n, seed + 1, device)
    full, out = fenced(device, n, shape[2])
    head.draws.fill_(77)
    head.act(obs, rows, out=out, deterministic=True)
    assert fence_holds(full) and bool(torch.isfinite(out).all())
    assert head.draws.cpu().tolist() == [77] * n   # a deterministic act leaves the counters alone
    want = pi64(ref, obs, rows)
    assert 0.05 <= float(np.abs(want).mean()) <= 0.95, float(np.abs(want).mean())   # tanh neither linear nor saturated
    err = float(np.abs(out.cpu().double().numpy() - want).max())
    head.close(), agent.close()
    return err


def check_forward(lib, device, shape, n):
    err = forward_error(lib, device, shape, n, 3 + shape[0] + n)
    print("(D, G, A) = {}, N = {}: max |action - float64| = {:.3e}".format(shape, n, err))
    assert err <= ACTION_TOL, (shape, n, err)


# ---- 2, 3 --------------------------------------------------------------------------------------------------------------------
def reference_draws(seed, ids, counter):
    """The numpy restatement of the exploration draws: (normals [N, 4], uniforms 2 u - 1 [N, 4], decision word [N])."""
    normals = oph.box_muller(oph.rng_bits(seed, ids, counter, STREAM, sub=0))
    uniforms = 2.0 * oph.u01(oph.rng_bits(seed, ids, counter, STREAM, sub=1)) - 1.0
    word = oph.rng_bits(seed, ids, counter, STREAM, sub=2)[:, 0].astype(np.uint64)
    return normals, uniforms, word


def box_muller_error(lib, device, n, seed):
    """The error of the device box_muller, on code this head does not touch: the existing rollout head (fwg_actor_act) with zero
    weights and log_std 0 returns its noise as its action."""
    import test_actor_contract as tac
    from emu.host_backend import HostBackend
    from gym_fixed_wing.vec_env import _TorchBackend
    mem = HostBackend() if torch.device(device).type == "cpu" else _TorchBackend(0)
    A, D = 4, 9
    w = {k: np.zeros_like(v) for k, v in tac._weights(D, A, 1).items()}
    head = tac._Head(lib, mem, n, D, A, w, training=False, seed=seed, env_id_base=0)
    got = head.step(np.zeros((n, D), np.float32), deterministic=False, observe=False)["action"].astype(np.float64)
    head.close()
    want = oph.box_muller(oph.rng_bits(seed, np.arange(n), 0, tac.STREAM_POLICY))
    return float(np.abs(got - want).max())


def check_draws(lib, device):
    """eps = 0.3, N = 130, three consecutive acts: the decision per env, the uniform actions, the Gaussian ones, the counters."""
    shape, n, seed, base, sigma = (11, 3, 4), 130, (5 << 32) | 9, 1000, 0.2
    agent, ref = make_agent(lib, device, shape, 41)
    head = BehaviourHead(agent, n, seed=seed, env_id_base=base, noise=sigma, random_eps=0.3, _lib=lib)
    bm = box_muller_error(lib, device, n, 17)
    tol = ACTION_TOL + sigma * 2.0 * bm
    print("box_muller error of the existing head over {} draws: {:.3e}; Gaussian tolerance {:.3e}".format(4 * n, bm, tol))
    seen = 0
    for c in range(3):
        obs, rows = inputs(shape, n, 50 + c, device)
        full, out = fenced(device, n, shape[2])
        head.act(obs, rows, out=out)
        assert fence_holds(full)
        got = out.cpu().double().numpy()
        normals, uniforms, word = reference_draws(seed, base + np.arange(n), c)
        random = word < np.uint64(eps_scaled(0.3))
        is_uniform = (np.abs(got - uniforms) <= UNIFORM_TOL).all(axis=1)
        np.testing.assert_array_equal(is_uniform, random)   # the decision, exact per env
        gauss = np.clip(pi64(ref, obs, rows) + sigma * normals, -1.0, 1.0)
        assert np.abs(got - gauss)[~random].max() <= tol, float(np.abs(got - gauss)[~random].max())
        seen += int(random.sum())
    assert 0.15 * 3 * n <= seen <= 0.45 * 3 * n, seen
    assert head.draws.cpu().tolist() == [3] * n
    for eps, want_all in ((1.0, True), (0.0, False)):
        head.set_noise(sigma, eps)
        assert int(head.noise_params.cpu().view(torch.int32)[2]) == (1 if eps == 1.0 else 0)   # eps_scaled = 2^32: its high word
        c = int(head.draws[0])
        obs, rows = inputs(shape, n, 60, device)
        got = head.act(obs, rows).cpu().double().numpy()
        _, uniforms, _ = reference_draws(seed, base + np.arange(n), c)
        is_uniform = (np.abs(got - uniforms) <= UNIFORM_TOL).all(axis=1)
        assert is_uniform.all() if want_all else not is_uniform.any()
    head.close(), agent.close()


def check_gaussian_clipping(lib, device):
    """sigma = 1.5: both branches of the clamp occur; clipped entries are +-1 exactly."""
    shape, n, seed, sigma = (11, 3, 4), 130, 123, 1.5
    agent, ref = make_agent(lib, device, shape, 43)
    head = BehaviourHead(agent, n, seed=seed, noise=sigma, random_eps=0.0, _lib=lib)
    obs, rows = inputs(shape, n, 70, device)
    full, out = fenced(device, n, shape[2])
    head.act(obs, rows, out=out)
    assert fence_holds(full)
    got = out.cpu().double().numpy()
    raw = pi64(ref, obs, rows) + sigma * oph.box_muller(oph.rng_bits(seed, np.arange(n), 0, STREAM, sub=0))
    clipped = np.abs(raw) > 1.0
    assert 0.1 <= clipped.mean() <= 0.9, float(clipped.mean())   # the condition, from the float64 reference alone
    bm = box_muller_error(lib, device, n, 17)
    tol = ACTION_TOL + sigma * 2.0 * bm
    print("box_muller error {:.3e}; tolerance {:.3e}; clipped share {:.2f}".format(bm, tol, clipped.mean()))
    assert np.abs(got - np.clip(raw, -1.0, 1.0)).max() <= tol
    sure = np.abs(raw) > 1.0 + tol   # (within the tolerance of the clip fp32 and float64 may fall on either side)
    np.testing.assert_array_equal(got[sure], np.sign(raw[sure]))
    assert np.abs(got).max() <= 1.0
    head.close(), agent.close()


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
def check_stream_independence(lib, device):
    shape, seed = (11, 3, 3), 99
    agent, _ = make_agent(lib, device, shape, 45)
    whole = BehaviourHead(agent, 130, seed=seed, env_id_base=0, noise=0.4, random_eps=0.25, _lib=lib)
    shard = BehaviourHead(agent, 65, seed=seed, env_id_base=65, noise=0.4, random_eps=0.25, _lib=lib)
    first = []
    for c in range(2):
        obs, rows = inputs(shape, 130, 80 + c, device)
        a, b = whole.act(obs, rows), shard.act(obs[65:].contiguous(), rows[65:].contiguous())
        assert same(a[65:], b)
        first.append(a.clone())
    assert not same(first[0], first[1])
    # a deterministic act neither reads nor writes the counters: whatever they hold, the same actions and the same counters
    obs, rows = inputs(shape, 130, 80, device)
    before = whole.draws.clone()
    det = whole.act(obs, rows, deterministic=True).clone()
    assert same(whole.draws, before)
    whole.draws.copy_(torch.arange(130, dtype=torch.int32) * 7919 - 5)
    pattern = whole.draws.clone()
    assert same(whole.act(obs, rows, deterministic=True), det) and same(whole.draws, pattern)
    # reseed restarts the stream bit for bit
    whole.reseed(seed)
    assert whole.draws.cpu().tolist() == [0] * 130
    assert same(whole.act(obs, rows), first[0])
    whole.reseed(seed + 1)
    assert not same(whole.act(obs, rows), first[0])
    whole.close(), shard.close(), agent.close()


# ---- 5, 6 --------------------------------------------------------------------------------------------------------------------
def make_env(env_kw, n, seed=0, steps_max=25, cfg=None, **kw):
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    return FixedWingVecEnv(oc.her_config() if cfg is None else cfg, num_envs=n, seed=seed, config_kw={"steps_max": steps_max}, **dict(env_kw, **kw))


def guarded(m, n, cols=None, kind="f32"):
    """fenced() in the env's memory: (full, view)."""
    full = m.full((n + 1,) if cols is None else (n + 1, cols), 255 if kind == "u8" else float("nan"), kind)
    return full, full[:n]


def guard_holds(m, full):
    last = np.asarray(m.to_host(full))[-1]
    return bool((last == 255).all()) if last.dtype == np.uint8 else bool(np.isnan(last).all())


def check_goal_rows(lib, device, env_kw):
    """With an env handle: the rows are fwg_goal_observe's bit for bit, the actions those of the env-less call fed those rows."""
    from gym_fixed_wing import goal
    n = 130
    vec = make_env(env_kw, n)
    m, D = vec._mem, vec.obs_dim
    spec = goal.GoalSpec.from_env(vec)
    st = spec.struct(0)
    agent, _ = make_agent(lib, device, (D, spec.n, 3), 47)
    with_env = BehaviourHead(agent, n, seed=5, noise=0.3, random_eps=0.2, _lib=lib)
    free = BehaviourHead(agent, n, seed=5, noise=0.3, random_eps=0.2, _lib=lib)
    rng = np.random.default_rng(1)
    vec.reset()
    for stage in range(2):
        for _ in range(3 * stage):
            vec.step_device(m.from_host(rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)))
        ach, des = m.zeros((n, 4)), m.zeros((n, 4))
        goal._observe(vec, st, ach, des)
        (fa, a), (fd, d), (fo, o), (fx, x), (ff, f) = guarded(m, n, 4), guarded(m, n, 4), guarded(m, n, D), guarded(m, n, 3), guarded(m, n, None, "u8")
        with_env.act_env(vec, st, a, d, o, x, f)
        m.sync()
        assert all(guard_holds(m, t) for t in (fa, fd, fo, fx, ff))
        assert same(m.to_host(a), m.to_host(ach)) and same(m.to_host(d), m.to_host(des))
        assert same(m.to_host(o), m.to_host(vec._obs)) and same(m.to_host(f), m.to_host(vec._done))
        assert np.abs(np.asarray(m.to_host(des))[:, :spec.n]).max() > 0.0
        want = free.act(vec._obs, des)
        m.sync()
        assert same(m.to_host(x), m.to_host(want))
    with_env.close(), free.close(), agent.close(), vec.close()


def parts_rollout(vec, head, log, T):
    """One rollout written out of the parts: BehaviourHead.act (env-less), vec.step_device, GoalLog.observe and copies."""
    m, N, D = vec._mem, vec.num_envs, vec.obs_dim
    buf = {"obs": m.zeros((T, N, D)), "actions": m.zeros((T, N, 3)), "raw_rewards": m.zeros((T, N)), "dones": m.zeros((T, N), "u8")}
    cur = {"obs": m.zeros((N, D)), "actions": m.zeros((N, 3))}
    log.observe(0)
    buf["obs"][0][...] = vec._obs
    head.act(vec._obs, log.desired[0], out=buf["actions"][0])
    for t in range(T):
        _, _, d = vec.step_device(buf["actions"][t], reward_out=buf["raw_rewards"][t])
        buf["dones"][t][...] = d
        log.observe(t + 1)
        nxt = cur if t == T - 1 else {"obs": buf["obs"][t + 1], "actions": buf["actions"][t + 1]}
        nxt["obs"][...] = vec._obs
        head.act(vec._obs, log.desired[t + 1], out=nxt["actions"])
    return buf, cur


def equal_rollouts(m, a, b):
    (buf_a, cur_a, log_a), (buf_b, cur_b, log_b) = a, b
    for k in ("obs", "actions", "raw_rewards", "dones"):
        assert same(m.to_host(buf_a[k]), m.to_host(buf_b[k])), k
    for k in ("obs", "actions"):
        assert same(m.to_host(cur_a[k]), m.to_host(cur_b[k])), "cur " + k
    assert same(m.to_host(log_a.achieved), m.to_host(log_b.achieved)) and same(m.to_host(log_a.desired), m.to_host(log_b.desired))


def check_collector(lib, device, env_kw):
    """HindsightCollector.run() against the loop of its parts over two consecutive rollouts with an episode end among them, then
    the replay buffer and both learners behind it."""
    from gym_fixed_wing.goal import GoalLog
    from gym_fixed_wing.replay import HindsightReplay
    N, T = 130, 4
    for path in ("hip", "torch"):
        vec, twin = make_env(env_kw, N, seed=3, steps_max=6), make_env(env_kw, N, seed=3, steps_max=6)
        m, D = vec._mem, vec.obs_dim
        agent = DDPG(D, 3, 3, update=path, device=device, seed=11, _lib=lib)
        col = HindsightCollector(vec, agent, T, seed=21, noise=0.3, random_eps=0.2, _lib=lib)
        head = BehaviourHead(agent, N, seed=21, noise=0.3, random_eps=0.2, _lib=lib)
        log = GoalLog(twin, T)
        replay = HindsightReplay(vec, T, 2, seed=1)
        vec.reset(), twin.reset()
        any_done = False
        for _ in range(2):
            col.run()
            buf, cur = parts_rollout(twin, head, log, T)
            m.sync()
            equal_rollouts(m, (col.buf, col.cur, col.goals), (buf, cur, log))
            any_done = any_done or bool(np.asarray(m.to_host(buf["dones"])).any())
            assert replay.add_rollout(col) in (0, 1)
        assert any_done   # the condition: an episode ended inside the two rollouts
        assert np.abs(np.asarray(m.to_host(col.buf["actions"]))).max() <= 1.0 and col.head.draws.cpu().tolist() == [2 * (T + 1)] * N
        # the learner behind the buffer; the head follows an update in place (hip), or at refresh() (torch)
        det = lambda: bits(head.act(vec._obs, col.goals.desired[T], deterministic=True)).clone()
        before = det()
        stats = agent.update(replay.sample(257))
        assert all(np.isfinite(v) for v in stats.values())
        if path == "torch":
            assert torch.equal(det(), before)   # without refresh() the head acts on the old weights
            head.refresh()
        after = det()
        assert not torch.equal(after, before)
        fresh = BehaviourHead(agent, N, _lib=lib)
        assert torch.equal(bits(fresh.act(vec._obs, col.goals.desired[T], deterministic=True)), after)
        for x in (head, fresh, col.head, agent, vec, twin):
            x.close()


# ---- 7 (GPU only) ------------------------------------------------------------------------------------------------------------
def check_graph_replay(lib, device, env_kw):
    from gym_fixed_wing.replay import HindsightReplay
    N, T = 130, 4
    vec, twin = make_env(env_kw, N, seed=3, steps_max=9), make_env(env_kw, N, seed=3, steps_max=9)
    m, D = vec._mem, vec.obs_dim
    agent = DDPG(D, 3, 3, update="hip", device=device, seed=11, _lib=lib)
    vec.reset(), twin.reset()
    kw = dict(seed=21, noise=0.3, random_eps=0.2, _lib=lib)
    graphed, eager = HindsightCollector(vec, agent, T, graph=True, **kw), HindsightCollector(twin, agent, T, **kw)
    warm = eager.warm_up()
    m.sync()
    assert same(graphed.warmup[0], warm[0]) and same(graphed.warmup[1], warm[1])
    probe = BehaviourHead(agent, N, _lib=lib)
    replay = HindsightReplay(vec, T, 2, seed=1)
    done = False

    def both():
        nonlocal done
        graphed.run(), eager.run()
        m.sync()
        equal_rollouts(m, (graphed.buf, graphed.cur, graphed.goals), (eager.buf, eager.cur, eager.goals))
        done = done or bool(graphed.buf["dones"].any())
    for _ in range(3):
        both()
    assert done and graphed.head.draws.cpu().tolist() == [3 + 3 * (T + 1)] * N
    replay.add_rollout(graphed)
    # set_noise between replays, no recapture: eps = 1 makes every action uniform, sigma = 0 and eps = 0 leave pi itself
    for c in (graphed, eager):
        c.head.set_noise(0.3, 1.0)
    c0 = int(graphed.head.draws[0])
    both()
    _, uniforms, _ = reference_draws(21, np.arange(N), c0)
    assert np.abs(graphed.buf["actions"][0].cpu().double().numpy() - uniforms[:, :3]).max() <= UNIFORM_TOL
    for c in (graphed, eager):
        c.head.set_noise(0.0, 0.0)
    both()
    pi = lambda: probe.act(graphed.buf["obs"][0], graphed.goals.desired[0], deterministic=True)
    assert same(graphed.buf["actions"][0], pi())
    # an update between replays: the next rollout acts on the new weights (slice 0 acts on the observation cur holds)
    old = probe.act(graphed.cur["obs"], graphed.goals.desired[T], deterministic=True).clone()
    agent.update(replay.sample(257))
    both()
    assert same(graphed.buf["actions"][0], pi()) and not same(graphed.buf["actions"][0], old)
    for x in (probe, graphed.head, eager.head, agent):
        x.close()
    vec.set_graph_mode(False)
    vec.close(), twin.close()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, device, env_kw, row_log_kw):
    from gym_fixed_wing import goal, presets
    n = 5
    null, p = ctypes.c_void_p(), lambda t: ctypes.c_void_p(int(t.data_ptr()))
    z = lambda *s, **k: torch.zeros(*s, device=device, **k)
    params, obs, rows, act, draws, noise = z(20000), z(n, 64), z(n, 4), z(n, 4), z(n, dtype=torch.int32), z(4, dtype=torch.int32)

    def call(D, G, A, env=null, spec=None, goal_rows=rows, ach=null, des=null, N=n, obs_=obs):
        return lambda: nat.check(lib, lib.fwg_behaviour_act(env, spec, N, D, G, A, p(params), p(obs_) if obs_ is not None else null,
                                                            p(goal_rows) if goal_rows is not None else null, ach, des, null, p(act), null, null,
                                                            p(draws), p(noise), 0, 0, 1, null))
    oc.native_error(call(62, 3, 1), "D + G")
    oc.native_error(call(62, 3, 1), "D 62, G 3, A 1")
    oc.native_error(call(58, 3, 4), "D + G + A")
    oc.native_error(call(11, 5, 3), "G must")
    oc.native_error(call(11, 0, 3), "G must")
    oc.native_error(call(11, 3, 5), "A must")
    oc.native_error(call(11, 3, 0), "A must")
    oc.native_error(call(11, 3, 3, goal_rows=None), "neither env nor goal_rows")
    oc.native_error(call(11, 3, 3, obs_=None), "obs")
    oc.native_error(call(11, 3, 3, N=0), "N must")
    vec = make_env(env_kw, n)
    spec = goal.GoalSpec.from_env(vec)
    st = spec.struct(0)
    m = vec._mem
    ach, des = m.zeros((n, 4)), m.zeros((n, 4))
    oc.native_error(call(11, 3, 3, env=vec._handle, spec=ctypes.byref(st), ach=m.ptr(ach), des=m.ptr(des)), "both env and goal_rows")
    oc.native_error(call(11, 3, 3, env=vec._handle, spec=ctypes.byref(st), goal_rows=None, des=m.ptr(des)), "achieved_out")
    oc.native_error(call(12, 3, 3, env=vec._handle, spec=ctypes.byref(st), goal_rows=None, ach=m.ptr(ach), des=m.ptr(des)), "D is 12")
    oc.native_error(call(11, 3, 3, env=vec._handle, spec=ctypes.byref(st), goal_rows=None, ach=m.ptr(ach), des=m.ptr(des), N=4), "N is 4")
    agent = DDPG(11, 3, 3, update="hip", device=device, _lib=lib)
    wide, other_goal = DDPG(12, 3, 3, device=device), DDPG(11, 2, 3, device=device)
    oc.value_error(lambda: HindsightCollector(vec, agent, 3, graph=True, _lib=lib), "n_steps must be even")
    oc.value_error(lambda: HindsightCollector(vec, wide, 4, _lib=lib), "(12, 3, 3)")
    oc.value_error(lambda: HindsightCollector(vec, other_goal, 4, _lib=lib), "(11, 2, 3)")
    oc.value_error(lambda: HindsightCollector(vec, agent, 4, head=BehaviourHead(agent, n + 1, _lib=lib)), "num_envs {}".format(n + 1))
    oc.value_error(lambda: BehaviourHead(DDPG(58, 3, 4, device=device), n, _lib=lib), "obs_dim 58, goal_dim 3, act_dim 4")
    head = BehaviourHead(agent, n, _lib=lib)
    oc.value_error(lambda: head.act(z(n, 12), z(n, 4)), "obs")
    oc.value_error(lambda: head.act(z(n, 11), z(n, 3)), "desired_rows")
    oc.value_error(lambda: head.act(z(n, 11), z(n, 4), out=z(n, 3, dtype=torch.float64)), "out")
    oc.value_error(lambda: head.set_noise(0.2, 1.5), "random_eps")
    oc.value_error(lambda: head.set_noise(-1.0, 0.0), "noise")
    # what GoalLog refuses comes through: a configuration without goals
    plain = make_env(env_kw, n, cfg=presets.preset("default"))
    oc.value_error(lambda: HindsightCollector(plain, agent, 4, _lib=lib), "observation.goals")
    # a row-log env, by the collector and by the C entry
    logged = make_env(row_log_kw, n, cfg=presets.preset("cnn"), obs_layout="row_log")
    assert logged.obs_log_rows > 0
    oc.value_error(lambda: HindsightCollector(logged, agent, 4, _lib=lib), "row log")
    one = nat.GoalSpecStruct()
    one.n_goals, one.var[0], one.inv_var[0] = 1, 1.0, 1.0
    lm = logged._mem
    oc.native_error(call(logged.obs_dim, 1, 3, env=logged._handle, spec=ctypes.byref(one), goal_rows=None, ach=lm.ptr(lm.zeros((n, 4))),
                         des=lm.ptr(lm.zeros((n, 4)))), "obs_log_rows")
    for x in (head, agent, vec, plain, logged):
        x.close()
