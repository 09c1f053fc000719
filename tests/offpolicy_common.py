"""Shared pieces of tests/test_offpolicy.py: the off-policy update (include/fwgym.h "Off-policy update", gym_fixed_wing/offpolicy.py)
on the host emulation of the kernels and on the GPU.  Every body takes (lib, device): the emulation library with "cpu", or the HIP
library with cuda:0.

Inputs: seeded synthetic batches, generated in float64 and rejected row by row until, with the fp32-rounded parameters, every ReLU
pre-activation of every network evaluation of the update is >= 1e-3 away from 0 and (twin critics) the two target values are >= 1e-3
apart: a unit whose sign differs between fp32 and float64 changes its gradient for that row by order 1 / B, which would test the
inputs and not the kernel.  That is a cap on the inputs, not a tolerance.  With torch's default initialisation as it stands the 128
hidden units of seven network evaluations leave ~25 % of the rows standing per pass (layer 2's pre-activations have a standard
deviation of ~0.35), so the WEIGHTS are scaled, not the threshold: both hidden layers' weights and biases by HIDDEN_SCALE, the output
layers down by its square -- the outputs stay of the same order -- and the actor's up again so that tanh is neither linear nor
saturated.  offpolicy tests check that at most half of the rows are rejected per pass for every shape.

Bounds: gradients <= 1e-4 relative Frobenius error per parameter tensor against float64 autograd of ddpg_losses, with the floor of
tests/test_ppo_hip.py::_compare for vanishing tensors; statistics within 1e-5 relative: of the statistic itself for
critic_loss, and for the three means of terms of both signs (actor_loss, q_mean, target_mean) of the mean magnitude of their terms, mean |Q_i| or
mean |y_i| -- test_ppo_hip.py's rule for pg_loss.  With the last layers as initialised a critic's value is a remainder of ~0.01 of 64 products that add up
to ~1 in magnitude, which no fp32 evaluation holds to 1e-5 of itself; a critic that has learnt anything is not there, so the INPUTS are moved and not the
bound: the online critics' last bias is raised by Q_OFFSET and the target critics' lowered by Q_OFFSET_TARGET (the same for both twins, so which of
them is the smaller still depends on the row), and the rewards are negative (-0.3 - 0.8 |n|), so Q - y is of order 1 on every row.  Adam against torch.optim.Adam with _check_apply's closeness; whole updates with _check_composed's."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from gym_fixed_wing import _native as nat
from gym_fixed_wing.offpolicy import DDPG, STAT_KEYS, GoalActor, GoalCritic, HipDDPG, ddpg_losses

GAMMA = 0.98
HIDDEN_SCALE = 4.0
SHAPES = [(11, 3, 3), (13, 3, 3), (57, 3, 4)]
EPS = 1e-3
Q_OFFSET, Q_OFFSET_TARGET = 0.7, 0.6


def make_nets(D, G, A, NC, seed):
    """(actor, critics, actor_target, critics_target): independent draws of torch's default initialisation, scaled as the module
    docstring says."""
    torch.manual_seed(seed)
    nets = [GoalActor(D, G, A), [GoalCritic(D, G, A) for _ in range(NC)], GoalActor(D, G, A), [GoalCritic(D, G, A) for _ in range(NC)]]
    with torch.no_grad():
        for m in [nets[0], nets[2]] + nets[1] + nets[3]:
            for i in (0, 2):
                m.net[i].weight.mul_(HIDDEN_SCALE)
                m.net[i].bias.mul_(HIDDEN_SCALE)
            m.net[4].weight.mul_((3.0 if isinstance(m, GoalActor) else 1.0) / HIDDEN_SCALE ** 2)
        # (the critics' values away from 0, as a critic's are once it has learnt anything: online + Q_OFFSET, target - Q_OFFSET_TARGET)
        for c in nets[1]:
            c.net[4].bias.add_(Q_OFFSET)
        for c in nets[3]:
            c.net[4].bias.sub_(Q_OFFSET_TARGET)
    return nets


def _preacts(net, x):
    """Both hidden layers' pre-activations of an nn.Sequential(Linear, ReLU, Linear, ReLU, Linear[, Tanh]) and its output."""
    z1 = net[0](x)
    z2 = net[2](torch.relu(z1))
    out = net[4](torch.relu(z2))
    return z1, z2, (torch.tanh(out) if len(net) > 5 else out)


def _rows_ok(nets64, o, o2, g, a):
    """Per row: every ReLU pre-activation of every network evaluation of one update >= EPS away from 0; twin targets >= EPS apart."""
    actor, critics, actor_t, critics_t = nets64
    ok = torch.ones(o.shape[0], dtype=torch.bool)

    def run(net, x):
        nonlocal ok
        z1, z2, out = _preacts(net, x)
        ok = ok & (z1.abs() >= EPS).all(1) & (z2.abs() >= EPS).all(1)
        return out
    with torch.no_grad():
        a2 = run(actor_t.net, torch.cat([o2, g], 1))
        q2 = [run(c.net, torch.cat([o2, g, a2], 1)).squeeze(1) for c in critics_t]
        if len(q2) > 1:
            ok = ok & ((q2[0] - q2[1]).abs() >= EPS)
        for c in critics:
            run(c.net, torch.cat([o, g, a], 1))
        pi = run(actor.net, torch.cat([o, g], 1))
        run(critics[0].net, torch.cat([o, g, pi], 1))
    return ok


def make_batch(nets, B, seed, counts=None):
    """A batch dict as HindsightReplay.sample returns it (desired_rows [B][4] with word 3 = 0, done uint8 on about a quarter of the
    rows, rewards of order 1), its rows rejected as the module docstring says.  counts: a list that receives (rows drawn, rows
    rejected) per pass."""
    D, G, A = nets[0].obs_dim, nets[0].goal_dim, nets[0].act_dim
    nets64 = [copy.deepcopy(nets[0]).double(), [copy.deepcopy(c).double() for c in nets[1]], copy.deepcopy(nets[2]).double(),
              [copy.deepcopy(c).double() for c in nets[3]]]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    o, o2, g, a = torch.empty(B, D, dtype=torch.float64), torch.empty(B, D, dtype=torch.float64), torch.empty(B, G, dtype=torch.float64), \
        torch.empty(B, A, dtype=torch.float64)
    todo = torch.ones(B, dtype=torch.bool)
    for _ in range(200):
        k = int(todo.sum())
        o[todo], g[todo] = rnd(k, D) * 1.5, rnd(k, G)
        o2[todo] = o[todo] + 0.3 * rnd(k, D)
        a[todo] = (rnd(k, A) * 0.6).clamp(-1, 1)
        # (the conditions are decided on the values the kernels see: the fp32-rounded rows)
        f = lambda x: x.float().double()
        bad = ~_rows_ok(nets64, f(o), f(o2), f(g), f(a))
        if counts is not None:
            counts.append((k, int((bad & todo).sum())))
        todo = todo & bad
        if not todo.any():
            break
    assert not todo.any(), "the rejection loop did not terminate"
    # (rewards of order 1 and negative, as the env's are: y stays below the online critics' values, so no row's Q - y is a cancelled
    # remainder -- with one row, critic_loss IS that row's (Q - y)^2)
    r = -0.3 - 0.8 * rnd(B).abs()
    done = (torch.rand(B, generator=gen) < 0.25).to(torch.uint8)
    rows = torch.zeros(B, 4)
    rows[:, :G] = g.float()
    return {"observation": o.float().contiguous(), "next_observation": o2.float().contiguous(), "action": a.float().contiguous(),
            "desired_rows": rows.contiguous(), "reward": r.float().contiguous(), "done": done.contiguous()}


def to_device(b, device):
    return {k: v.to(device) for k, v in b.items()}


def learner(lib, nets, device, **kw):
    """HipDDPG over copies of `nets` on `device`: online parameters from nets[0:2], target parameters from nets[2:4]."""
    actor, critics = copy.deepcopy(nets[0]).to(device), [copy.deepcopy(c).to(device) for c in nets[1]]
    L = HipDDPG(lib, actor, critics, kw.get("gamma", GAMMA), kw.get("tau", 0.05), 1e-3, 1e-3, 1, kw.get("max_grad_norm"), device)
    L.target.copy_(torch.cat([p.detach().reshape(-1) for m in [nets[2]] + nets[3] for p in m.parameters()]).to(device))
    return L


def ref_grads(nets, b):
    """float64 autograd of ddpg_losses on the fp32 data: ([critic gradients], [actor gradients], statistics, magnitudes, y)."""
    n64 = [copy.deepcopy(nets[0]).double(), [copy.deepcopy(c).double() for c in nets[1]], copy.deepcopy(nets[2]).double(),
           [copy.deepcopy(c).double() for c in nets[3]]]
    G = nets[0].goal_dim
    o, o2, a, g, r = (b[k].double() for k in ("observation", "next_observation", "action", "desired_rows", "reward"))
    g, done = g[:, :G], b["done"].double()
    lc, la, st = ddpg_losses(n64[0], n64[1], n64[2], n64[3], o, o2, a, g, r, done, GAMMA)
    cp = [p for c in n64[1] for p in c.parameters()]
    gc_ = torch.autograd.grad(lc, cp, retain_graph=True)
    ga = torch.autograd.grad(la, list(n64[0].parameters()))
    with torch.no_grad():
        a2 = n64[2](o2, g)
        y = r + GAMMA * (1.0 - done) * torch.stack([c(o2, g, a2) for c in n64[3]]).min(0).values
        # a mean of terms of both signs is held relative to the mean magnitude of its terms: test_ppo_hip.py's rule for pg_loss
        scale = {"critic_loss": abs(float(st["critic_loss"])), "actor_loss": float(n64[1][0](o, g, n64[0](o, g)).abs().mean()),
                 "q_mean": float(n64[1][0](o, g, a).abs().mean()), "target_mean": float(y.abs().mean())}
    return list(gc_), list(ga), {k: float(v) for k, v in st.items()}, scale, y


def compare(got, names, want):
    """<= 1e-4 relative Frobenius error per parameter tensor (a vanishing one within 1e-8 absolute): test_ppo_hip.py's _compare."""
    g = got.cpu().double()
    o = 0
    for name, w in zip(names, want):
        x = g[o:o + w.numel()].view_as(w)
        o += w.numel()
        err = float((x - w).norm() / max(float(w.norm()), 1e-4))
        print("  {:<24s} rel. Frobenius error {:.3e}".format(name, err))
        assert err <= 1e-4, (name, err)
    assert o == g.numel()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


SENTINEL = -7.25


def check_grads(lib, device, B, shape, NC, seed):
    """Check 1: both gradient launches against float64 autograd, the segments each leaves alone, the four statistics."""
    D, G, A = shape
    nets = make_nets(D, G, A, NC, seed)
    b = make_batch(nets, B, seed + 1)
    want_c, want_a, st_want, scale, _ = ref_grads(nets, b)
    L = learner(lib, nets, device)
    db = to_device(b, device)
    bs = L.batch_struct(db)
    PA, P = L.actor_params, L.num_params
    gc_ = torch.full((P + nat.DDPG_NSTAT,), SENTINEL, device=device)
    ga = torch.full((P + nat.DDPG_NSTAT,), SENTINEL, device=device)
    L.critic_grad(bs, B, gc_)
    L.actor_grad(bs, B, ga)
    sent = bits(torch.full((P + nat.DDPG_NSTAT,), SENTINEL))
    # the actor launch leaves the critics' gradient words (and their loss sums) untouched, bit for bit; and the reverse
    assert torch.equal(bits(ga)[PA:P], sent[PA:P]) and torch.equal(bits(ga)[[P, P + 2, P + 3]], sent[:3])
    assert torch.equal(bits(gc_)[:PA], sent[:PA]) and torch.equal(bits(gc_)[P + 1], sent[0])
    names_a = ["actor." + k for k, _ in L.actor.named_parameters()]
    names_c = ["critic{}.{}".format(j, k) for j, c in enumerate(L.critics) for k, _ in c.named_parameters()]
    print("B = {}, (D, G, A) = {}, n_critics = {}".format(B, shape, NC))
    compare(gc_[PA:P], names_c, want_c)
    compare(ga[:PA], names_a, want_a)
    # the statistics through the apply half, on copies of the state
    stats = torch.zeros(4, device=device)
    for seg, gbuf in ((nat.DDPG_CRITICS, gc_), (nat.DDPG_ACTOR, ga)):
        L.apply(seg, gbuf, B, params=L.flat.clone(), m=L.exp_avg.clone(), v=L.exp_avg_sq.clone(), steps=L.steps.clone(), stats=stats)
    st = dict(zip(STAT_KEYS, stats.cpu().tolist()))
    for k in STAT_KEYS:
        print("  {:<12s} {:+.8e} want {:+.8e}  error / scale {:.2e}".format(k, st[k], st_want[k], abs(st[k] - st_want[k]) / scale[k]))
    for k in STAT_KEYS:
        assert abs(st[k] - st_want[k]) <= 1e-5 * scale[k], (k, st[k], st_want[k], scale[k])
    L.close()


def check_td_target(lib, device, B, shape, NC, seed):
    """Check 2: y is r itself on a row with done set, and on every row at gamma = 0; elsewhere it follows the float64 target."""
    D, G, A = shape
    nets = make_nets(D, G, A, NC, seed)
    b = make_batch(nets, B, seed + 1)
    b["done"][0] = 1
    b["done"][B - 1] = 1
    if B > 2:
        b["done"][B // 2] = 0
    _, _, _, scale, y_want = ref_grads(nets, b)
    db = to_device(b, device)
    for gamma in (GAMMA, 0.0):
        L = learner(lib, nets, device, gamma=gamma)
        y = torch.full((B,), SENTINEL, device=device)
        L.critic_grad(L.batch_struct(db), B, torch.zeros(L.num_params + nat.DDPG_NSTAT, device=device), td_target=y)
        rows = b["done"].bool() if gamma else torch.ones(B, dtype=torch.bool)
        assert rows.any() and torch.equal(bits(y)[rows], bits(b["reward"])[rows])
        if gamma:
            assert float((y.cpu().double() - y_want).abs().max()) <= 1e-5 * max(float(y_want.abs().max()), 1.0)
            assert B < 3 or not torch.equal(bits(y)[B // 2], bits(b["reward"])[B // 2])
        L.close()


def check_apply(lib, device, max_grad_norm=None):
    """Check 3: three Adam steps per segment and the Polyak pass against torch.optim.Adam and lerp_ in fp32 on the same gradients
    (test_ppo_hip.py::_check_apply's closeness); the other segment, its moments and its step counter bit-equal before and after;
    tau = 1 copies the online vector exactly and tau = 0 leaves the target as it is.  max_grad_norm: clip_grad_norm_ per segment
    (both critics under one norm) before each step -- the gradients' norms are ~17 / 12, ~0.035 / 0.024 and ~3.5 / 2.4 (critics /
    actor), above and below 0.5."""
    nets = make_nets(11, 3, 3, 2, 5)
    L = learner(lib, nets, device, max_grad_norm=max_grad_norm)
    PA, P = L.actor_params, L.num_params
    ref = [copy.deepcopy(nets[0]).to(device)] + [copy.deepcopy(c).to(device) for c in nets[1]]
    ref_t = torch.cat([p.detach().reshape(-1) for m in [nets[2]] + nets[3] for p in m.parameters()]).to(device)
    segs = {nat.DDPG_ACTOR: (0, PA, list(ref[0].parameters())), nat.DDPG_CRITICS: (PA, P, [p for c in ref[1:] for p in c.parameters()])}
    gen = torch.Generator().manual_seed(9)
    close = lambda x, y, msg, atol=1e-7: np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().cpu().numpy(), rtol=1e-6, atol=atol, err_msg=msg)
    for seg in (nat.DDPG_CRITICS, nat.DDPG_ACTOR):
        lo, hi, plist = segs[seg]
        opt = torch.optim.Adam(plist, lr=1e-3)
        other = slice(PA, P) if seg == nat.DDPG_ACTOR else slice(0, PA)
        before = [bits(t)[other].clone() for t in (L.flat, L.exp_avg, L.exp_avg_sq)] + [bits(L.steps)[1 - seg].clone()]
        for step, scale in enumerate([5.0, 0.01, 1.0]):
            grads = [torch.randn(p.shape, generator=gen) * scale / 30 for p in plist]
            flat = torch.full((P + nat.DDPG_NSTAT,), float("nan"))   # (the other segment's gradient words are never read)
            flat[lo:hi] = torch.cat([x.reshape(-1) for x in grads])
            flat[P:] = 0.0
            last = step == 2
            L.apply(seg, flat.to(device), 64, polyak=last)
            for p, x in zip(plist, grads):
                p.grad = x.to(device).clone()
            if max_grad_norm is not None:
                norm = float(torch.nn.utils.clip_grad_norm_(plist, max_grad_norm))
                assert (norm > max_grad_norm) == (step != 1), (step, norm)
            opt.step()
            want = torch.cat([p.detach().reshape(-1) for p in plist])
            close(L.flat[lo:hi], want, "parameters, segment {} step {}".format(seg, step))
            for mine, key in ((L.exp_avg, "exp_avg"), (L.exp_avg_sq, "exp_avg_sq")):
                w = torch.cat([opt.state[q][key].reshape(-1) for q in plist])
                close(mine[lo:hi], w, key, atol=1e-6 * float(w.abs().max()))
            if last:
                ref_t.lerp_(torch.cat([p.detach().reshape(-1) for m in ref for p in m.parameters()]), 0.05)
                close(L.target, ref_t, "target after the Polyak pass")
        after = [bits(t)[other] for t in (L.flat, L.exp_avg, L.exp_avg_sq)] + [bits(L.steps)[1 - seg]]
        for x, y in zip(before, after):
            assert torch.equal(x, y)
    assert L.steps.cpu().tolist() == [3, 3]
    zero = torch.zeros(P + nat.DDPG_NSTAT, device=device)
    for tau in (0.0, 1.0):
        L.hparams.tau = tau
        t0 = L.target.clone()
        L.apply(nat.DDPG_ACTOR, zero, 64, polyak=True)
        assert torch.equal(bits(L.target), bits(t0 if tau == 0.0 else L.flat))
    assert not torch.equal(bits(t0), bits(L.flat))
    L.close()


def fixed_batches(shape, NC, B, n=8):
    D, G, A = shape
    nets = make_nets(D, G, A, NC, 21)
    return [make_batch(nets, B, 100 + i) for i in range(n)]


def run_updates(lib, device, path, batches, shape, **kw):
    D, G, A = shape
    agent = DDPG(D, G, A, update=path, device=device, seed=3, _lib=lib, **kw)
    w0 = agent.updater.params().cpu()
    stats, trail = [], []
    for b in batches:
        stats.append(agent.update(to_device(b, device)))
        trail.append((agent.updater.params().cpu(), agent.updater.target_params().cpu()))
    return agent, w0, stats, trail


def check_updates(lib, device, batches, shape, **kw):
    """Check 4: the HIP path against the torch path over the same batches from the same start (test_ppo_hip.py::_check_composed's
    bounds), the policy delay, and bitwise determinism of the HIP path."""
    at, w0, st_t, tr_t = run_updates(lib, device, "torch", batches, shape, **kw)
    ah, w0h, st_h, tr_h = run_updates(lib, device, "hip", batches, shape, **kw)
    assert torch.equal(w0, w0h)
    rel = float((tr_h[-1][0] - tr_t[-1][0]).norm() / (tr_t[-1][0] - w0).norm())
    rel_t = float((tr_h[-1][1] - tr_t[-1][1]).norm() / (tr_t[-1][1] - w0).norm())
    print("after {} updates: |w_hip - w_torch| / |w_torch - w_0| = {:.3e} (target: {:.3e})".format(len(batches), rel, rel_t))
    assert rel <= 1e-2 and rel_t <= 1e-2, (rel, rel_t)
    for u, (a, b) in enumerate(zip(st_h, st_t)):
        for k in STAT_KEYS:
            assert a[k] == pytest.approx(b[k], rel=2e-2, abs=1e-4), (u + 1, k, a[k], b[k])
    assert all(np.isfinite(s[k]) for s in st_h for k in STAT_KEYS)
    delay, PA = kw.get("policy_delay", 1), ah.updater.actor_params
    prev = (w0, w0)
    for u, (w, t) in enumerate(tr_h, 1):   # the actor and the targets move on the delayed updates only, the critics on every one
        moved_a, moved_t = not torch.equal(bits(w)[:PA], bits(prev[0])[:PA]), not torch.equal(bits(t), bits(prev[1]))
        assert moved_a == moved_t == (u % delay == 0), (u, moved_a, moved_t)
        assert not torch.equal(bits(w)[PA:], bits(prev[0])[PA:])
        prev = (w, t)
    assert ah.updater.steps.cpu().tolist() == [len(batches) // delay, len(batches)]
    ah2, _, _, tr_h2 = run_updates(lib, device, "hip", batches, shape, **kw)
    assert torch.equal(bits(tr_h[-1][0]), bits(tr_h2[-1][0])) and torch.equal(bits(tr_h[-1][1]), bits(tr_h2[-1][1]))
    for a in (at, ah, ah2):
        a.close()


def her_config():
    """examples/train_her.py's configuration."""
    from gym_fixed_wing import presets
    from gym_fixed_wing.replay import without_goal_targets
    cfg = presets.preset("default")
    cfg["observation"]["goals"] = [{"name": "roll", "mean": 0.0, "var": 1.0}, {"name": "pitch", "mean": 0.0, "var": 0.5},
                                   {"name": "Va", "mean": 22.0, "var": 10.0}]
    return without_goal_targets(cfg)


def check_end_to_end(lib, device, env_kw, n_envs, batch):
    """Check 5: a GoalVecEnv on train_her.py's configuration, two rollouts of 16 steps into a HindsightReplay, then four
    sample -> update rounds per path with equal seed and serial, under check 4's bound -- the 4-word goal stride, the uint8 done
    and the dict keys as sample really returns them."""
    from gym_fixed_wing.goal import GoalLog, GoalVecEnv
    from gym_fixed_wing.replay import HindsightReplay
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    vec = FixedWingVecEnv(her_config(), num_envs=n_envs, seed=0, config_kw={"steps_max": 25}, **env_kw)
    env = GoalVecEnv(vec)
    m, T, N, D, G = vec._mem, 16, n_envs, vec.obs_dim, env.spec.n
    assert (D, G) == (11, 3)
    log = GoalLog(vec, T)
    replay = HindsightReplay(vec, T, 2, strategy="future", p=0.8, seed=1)
    obs, actions, raw, dones = m.zeros((T, N, D)), m.zeros((T, N, 3)), m.zeros((T, N)), m.zeros((T, N), "u8")
    rng = np.random.default_rng(0)
    cur = env.reset()
    for _ in range(2):
        log.observe(0)
        for t in range(T):
            obs[t][...] = cur["observation"].reshape(N, D)
            actions[t][...] = m.from_host(rng.uniform(-1, 1, size=(N, 3)).astype(np.float32))
            cur, _, d = env.step_device(actions[t], reward_out=raw[t])
            dones[t][...] = d
            log.observe(t + 1)
        replay.add(obs, cur["observation"].reshape(N, D), actions, raw, dones, log)
    assert np.asarray(m.to_host(replay.dones)).any()
    agents = {p: DDPG(D, G, 3, update=p, device=device, seed=4, _lib=lib) for p in ("torch", "hip")}
    w0 = agents["torch"].updater.params().cpu()
    assert torch.equal(w0, agents["hip"].updater.params().cpu())
    stats = {"torch": [], "hip": []}
    for path, agent in agents.items():
        replay.serial = 0
        for _ in range(4):
            out = replay.sample(batch)
            assert out["done"].dtype in (np.uint8, torch.uint8) and tuple(out["desired_rows"].shape) == (batch, 4)
            stats[path].append(agent.update(out))
    wt, wh = agents["torch"].updater.params().cpu(), agents["hip"].updater.params().cpu()
    rel = float((wh - wt).norm() / (wt - w0).norm())
    print("end to end, {} envs: |w_hip - w_torch| / |w_torch - w_0| = {:.3e}".format(n_envs, rel))
    assert rel <= 1e-2, rel
    for a, b in zip(stats["hip"], stats["torch"]):
        for k in STAT_KEYS:
            assert np.isfinite(a[k]) and a[k] == pytest.approx(b[k], rel=2e-2, abs=1e-4), (k, a[k], b[k])
    for a in agents.values():
        a.close()
    vec.close()


def _refused(fn, kind, word):
    """(No exception object outlives this call: a kept traceback would hold `fn`'s learner in a reference cycle, and a learner freed by
    the garbage collector gives its device buffers back at a time nobody chose -- inside a later test's graph capture, for one.)"""
    try:
        fn()
    except kind as e:
        msg = str(e)
    else:
        raise AssertionError("no {} holding '{}'".format(kind.__name__, word))
    assert word in msg, (word, msg)


def native_error(fn, word):
    _refused(fn, nat.NativeError, word)


def value_error(fn, word):
    _refused(fn, ValueError, word)


def check_refusals(lib, device):
    """Check 6: each refusal names its argument."""
    h = ctypes.c_void_p()
    for D, G, A in ((58, 3, 4), (62, 3, 3), (200, 4, 4)):
        native_error(lambda: nat.check(lib, lib.fwg_offpolicy_create(D, G, A, 1, ctypes.byref(h))), "obs_words {}, goal_words {}, act_dim {}".format(D, G, A))
        value_error(lambda: DDPG(D, G, A, update="hip", device=device, _lib=lib), "obs_dim {}, goal_dim {}, act_dim {}".format(D, G, A))
    native_error(lambda: nat.check(lib, lib.fwg_offpolicy_create(11, 3, 3, 3, ctypes.byref(h))), "n_critics")
    native_error(lambda: nat.check(lib, lib.fwg_offpolicy_create(11, 5, 3, 1, ctypes.byref(h))), "goal_words")
    native_error(lambda: nat.check(lib, lib.fwg_offpolicy_create(11, 3, 0, 1, ctypes.byref(h))), "act_dim")
    native_error(lambda: nat.check(lib, lib.fwg_offpolicy_create(11, 3, 3, 1, None)), "out")
    value_error(lambda: DDPG(11, 3, 3, n_critics=3), "n_critics")
    value_error(lambda: DDPG(11, 3, 3, policy_delay=0), "policy_delay")
    value_error(lambda: DDPG(11, 3, 3, update="jax"), "update")
    nets = make_nets(11, 3, 3, 1, 1)
    b = to_device(make_batch(nets, 5, 2), device)
    other = to_device(make_batch(make_nets(12, 3, 3, 1, 1), 5, 2), device)
    for path in ("torch", "hip"):
        agent = DDPG(11, 3, 3, update=path, device=device, _lib=lib)
        value_error(lambda: agent.update(other), "observation")
        value_error(lambda: agent.update({k: v for k, v in b.items() if k != "desired_rows"}), "desired_rows")
        value_error(lambda: agent.update(dict(b, done=b["done"].float())), "done")
        assert agent.updates == 0
        if path == "torch":
            agent.close()
    # the C ABI: null pointers, B < 1, the policy delay and the segment, each by name
    L = agent.updater
    bs, p = L.batch_struct(b), lambda t: ctypes.c_void_p(int(t.data_ptr()))
    hp, null, st = ctypes.byref(L.hparams), ctypes.c_void_p(), L._stream()
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_critic_grad(L._h, ctypes.byref(bs), 0, hp, p(L.flat), p(L.target), p(L.grad), null, st)), "B ")
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_critic_grad(L._h, ctypes.byref(bs), 5, hp, p(L.flat), null, p(L.grad), null, st)), "target_params")
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_actor_grad(L._h, ctypes.byref(bs), 5, null, p(L.grad), st)), "params")
    bad = L.batch_struct(b)
    bad.goal_rows = None
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_actor_grad(L._h, ctypes.byref(bad), 5, p(L.flat), p(L.grad), st)), "batch.goal_rows")
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_apply(L._h, 2, p(L.grad), 5, hp, p(L.flat), p(L.exp_avg), p(L.exp_avg_sq), p(L.steps), p(L.stats), null, st)), "segment")
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_step(L._h, ctypes.byref(bs), 5, 1, 0, hp, p(L.flat), p(L.target), p(L.exp_avg), p(L.exp_avg_sq), p(L.steps),
                                                          p(L.stats), st)), "policy_delay")
    native_error(lambda: nat.check(lib, lib.fwg_ddpg_step(L._h, ctypes.byref(bs), 5, 1, 1, hp, p(L.flat), p(L.target), p(L.exp_avg), p(L.exp_avg_sq), null,
                                                          p(L.stats), st)), "steps")
    agent.close()
    agent.close()   # (a second close is a no-op)


def check_save_load(lib, device, tmp_path):
    nets = make_nets(11, 3, 3, 2, 1)
    b = to_device(make_batch(nets, 65, 2), device)
    agent = DDPG(11, 3, 3, n_critics=2, update="hip", device=device, seed=1, _lib=lib)
    agent.update(b)
    agent.save(str(tmp_path / "ddpg.npz"))
    o, g = b["observation"], b["desired_rows"][:, :3]
    a = agent.act(o, g).clone()
    other = DDPG(11, 3, 3, n_critics=2, update="hip", device=device, seed=2, _lib=lib)
    assert not torch.equal(other.act(o, g), a)
    other.load(str(tmp_path / "ddpg.npz"))
    # (the modules' parameters are views of the flat buffer: act() sees the loaded weights with no copy)
    assert torch.equal(other.act(o, g), a) and other.updates == 1
    assert torch.equal(bits(other.updater.target), bits(agent.updater.target))
    noisy = other.act(o, g, noise=0.3)
    assert float(noisy.abs().max()) <= 1.0 and not torch.equal(noisy, a)
    agent.close()
    other.close()
