"""Shared pieces of tests/test_offpolicy_contract.py: the off-policy update (csrc/fwgym_offpolicy.h, fwg_ddpg_*) against float64 over
its whole shape contract.  Every body takes (lib, device) as tests/offpolicy_common.py's do, whose networks, batches, float64
reference and bounds these are.

Inputs.  offpolicy_common's batches keep every ReLU pre-activation 1e-3 away from 0 and Q - y of order 1.  One more property of the
data decides what fp32 can hold of the ACTOR's gradient: dL_a / d(pre-tanh output k) of row i is -(1/B)(1 - p_ik^2) sum_j G1_ij W1_jk
(G1 = dQ_0 / d(pre-activation 1), W1's action columns), a dot product of terms of both signs, and the last bias' gradient is the sum
of it over the rows.  KAPPA = | sum_i (1/B)(1 - p_ik^2) sum_j |G1_ij W1_jk| | / | sum_i dL_a / dz_ik | (norms over k) says by how
much that sum is a cancelled remainder: the kernels' error divided by it is 1e-6 .. 7e-6 everywhere, so at KAPPA > 32 a one-row batch
or a one-element bias gradient would test the draw and not the kernel.  As with Q_OFFSET and the ReLU margin the inputs are moved and
not the bound: a case takes the first seed from its base seed upward (at most SEEDS_TRIED) whose KAPPA, computed in float64 from the
reference alone, is <= KAPPA_MAX.  No seed is ever chosen by what a kernel returns.

Every check prints one line "OFFPOLICY_CONTRACT ..." with its worst error before it asserts (profiles/offpolicy_contract_errors.txt)."""
import copy
import ctypes
import functools
import math

import numpy as np
import torch

import offpolicy_common as oc
from gym_fixed_wing import _native as nat
from gym_fixed_wing.offpolicy import STAT_KEYS, GoalActor, GoalCritic

# the shape contract: obs_words >= 1, goal_words 1..4, act_dim 1..4, Kc = D + G + A <= 64.  Kc 3, 9, 16, 17, 32, 33, 48, 49, 63, 64
# and Ka on both sides of 16, 32 and 48: the 16-column edges of ddpg_gather, the `tn0 < K` skip of ddpg_backward, ddpg_store's `n < K`
SHAPES = [(1, 1, 1), (1, 4, 4), (11, 4, 1), (12, 2, 2), (13, 1, 3), (27, 4, 1), (27, 2, 4), (28, 4, 1), (43, 4, 1), (44, 3, 2), (45, 2, 2),
          (58, 4, 1), (56, 4, 4), (59, 1, 4), (60, 3, 1), (62, 1, 1)]
BATCHES = [1, 63, 64, 65, 129]
KAPPA_MAX, SEEDS_TRIED = 32.0, 20
# one shape per goal width for the fenced buffers
FENCED_SHAPES = [(13, 1, 3), (12, 2, 2), (44, 3, 2), (56, 4, 4)]
# 321 tiles over the 256 workgroups: 65 workgroups take two tiles, and the last tile holds one row
SPLIT_B = 20481
# section 4's hyper-parameters: no two alike
LR_ACTOR, LR_CRITIC, MAXN_ACTOR, MAXN_CRITIC, BETAS, ADAM_EPS = 3e-4, 2e-3, 0.05, 0.5, (0.8, 0.99), 1e-5
STEPS0 = [2, 7]
FENCE = 64


def label(device):
    return "emu" if str(device) == "cpu" else "gpu"


def say(check, device, what, **figures):
    print("OFFPOLICY_CONTRACT {} {} {}: {}".format(check, label(device), what, " ".join("{}={:.3g}".format(k, v) for k, v in figures.items())))


def base_seed(shape, B, NC):
    D, G, A = shape
    return 1000 + 37 * D + 11 * G + 5 * A + 3 * B + 500 * NC


def kappa(nets, b):
    """KAPPA of the module docstring, in float64 -> (kappa, the true sum: the actor's last bias gradient)."""
    actor, c0 = copy.deepcopy(nets[0]).double(), copy.deepcopy(nets[1][0]).double()
    G, Ka = actor.goal_dim, actor.obs_dim + actor.goal_dim
    o, g = b["observation"].double(), b["desired_rows"][:, :G].double()
    with torch.no_grad():
        p = actor(o, g)
        z1, z2, _ = oc._preacts(c0.net, torch.cat([o, g, p], 1))
        W1a, W2, w3 = c0.net[0].weight[:, Ka:], c0.net[2].weight, c0.net[4].weight
        G1 = ((w3 * (z2 > 0)) @ W2) * (z1 > 0)   # [B][64] dQ_0 / d(pre-activation 1)
        f = (1.0 - p * p) / o.shape[0]
        true = -(f * (G1 @ W1a)).sum(0)
        mag = (f * (G1.abs() @ W1a.abs())).sum(0)
    return float(mag.norm() / true.norm()), true


class Case(object):
    """The inputs of one case and their float64 reference, made once and shared (never written to)."""

    def __init__(self, shape, B, NC):
        D, G, A = shape
        self.shape, self.B, self.NC = shape, B, NC
        self.kappas = []
        s0 = base_seed(shape, B, NC)
        for seed in range(s0, s0 + SEEDS_TRIED):
            nets = oc.make_nets(D, G, A, NC, seed)
            b = oc.make_batch(nets, B, seed + 1)
            k, true = kappa(nets, b)
            self.kappas.append(k)
            if k <= KAPPA_MAX:
                break
        self.seed, self.kappa, self.nets, self.b, self.bias_grad = seed, k, nets, b, true
        self.want_c, self.want_a, self.st_want, self.scale, self.y = oc.ref_grads(nets, b)

    def what(self):
        return "D={} G={} A={} B={} NC={} seed={}+{} kappa={:.3g}".format(*(self.shape + (self.B, self.NC, base_seed(self.shape, self.B, self.NC),
                                                                                         len(self.kappas) - 1, self.kappa)))


@functools.lru_cache(maxsize=None)
def case(shape, B, NC):
    return Case(shape, B, NC)


def set_hparams(L):
    h = L.hparams
    h.lr_actor, h.lr_critic, h.max_grad_norm_actor, h.max_grad_norm_critic = LR_ACTOR, LR_CRITIC, MAXN_ACTOR, MAXN_CRITIC
    h.beta1, h.beta2, h.eps = BETAS[0], BETAS[1], ADAM_EPS


def frobenius(got, names, want):
    """The worst relative Frobenius error over the parameter tensors (offpolicy_common.compare's: floor 1e-4 on the norm), with its name."""
    g = got.detach().cpu().double()
    o, worst = 0, (0.0, "")
    for name, w in zip(names, want):
        x = g[o:o + w.numel()].view_as(w)
        o += w.numel()
        worst = max(worst, (float((x - w).norm() / max(float(w.norm()), 1e-4)), name))
    assert o == g.numel()
    return worst


def names_of(L):
    return (["actor." + k for k, _ in L.actor.named_parameters()],
            ["critic{}.{}".format(j, k) for j, c in enumerate(L.critics) for k, _ in c.named_parameters()])


def fenced(b, G, device):
    """Every array of `b` as the contiguous slice [FENCE : FENCE + B] of a buffer whose other rows are NaN (`done`: 255, and the
    slice starts at an odd byte); words G..3 of every goal row NaN.  -> (batch, the buffers)"""
    B = int(b["reward"].shape[0])
    out, bufs = {}, []
    for k, v in b.items():
        if k == "done":
            buf = torch.full((B + 2 * FENCE + 1,), 255, dtype=torch.uint8)
            buf[FENCE + 1:FENCE + 1 + B] = v
            buf = buf.to(device)
            out[k] = buf[FENCE + 1:FENCE + 1 + B]
            assert out[k].data_ptr() % 2 == 1
        else:
            buf = torch.full((B + 2 * FENCE,) + tuple(v.shape[1:]), float("nan"))
            buf[FENCE:FENCE + B] = v
            if k == "desired_rows":
                buf[:, G:] = float("nan")
            buf = buf.to(device)
            out[k] = buf[FENCE:FENCE + B]
        assert out[k].is_contiguous()
        bufs.append(buf)
    return out, bufs


def launch_grads(L, db, B, device, y=None):
    """Both gradient launches into sentinel buffers, the statistics through the apply half on copies of the state.
    -> (critic launch's buffer, actor launch's buffer, statistics [4])"""
    P = L.num_params
    bs = L.batch_struct(db)
    gc_ = torch.full((P + nat.DDPG_NSTAT,), oc.SENTINEL, device=device)
    ga = torch.full((P + nat.DDPG_NSTAT,), oc.SENTINEL, device=device)
    L.critic_grad(bs, B, gc_, td_target=y)
    L.actor_grad(bs, B, ga)
    stats = torch.zeros(4, device=device)
    for seg, gbuf in ((nat.DDPG_CRITICS, gc_), (nat.DDPG_ACTOR, ga)):
        L.apply(seg, gbuf, B, params=L.flat.clone(), m=L.exp_avg.clone(), v=L.exp_avg_sq.clone(), steps=L.steps.clone(), stats=stats)
    return gc_, ga, stats


def assert_grads(check, device, c, L, gc_, ga, stats):
    """The launches' outputs of case `c` against its float64 reference: <= 1e-4 relative Frobenius error per tensor, the four
    statistics within 1e-5 of offpolicy_common's scales, the words each launch leaves alone bit-equal to the sentinel."""
    PA, P = L.actor_params, L.num_params
    sent = oc.bits(torch.full((P + nat.DDPG_NSTAT,), oc.SENTINEL))
    assert torch.equal(oc.bits(ga)[PA:P], sent[PA:P]) and torch.equal(oc.bits(ga)[[P, P + 2, P + 3]], sent[:3])
    assert torch.equal(oc.bits(gc_)[:PA], sent[:PA]) and torch.equal(oc.bits(gc_)[P + 1], sent[0])
    names_a, names_c = names_of(L)
    ec, ea = frobenius(gc_[PA:P], names_c, c.want_c), frobenius(ga[:PA], names_a, c.want_a)
    st = dict(zip(STAT_KEYS, stats.cpu().tolist()))
    es = max((abs(st[k] - c.st_want[k]) / c.scale[k], k) for k in STAT_KEYS)
    say(check, device, c.what(), frobenius=max(ec, ea)[0], statistic=es[0])
    assert ec[0] <= 1e-4 and ea[0] <= 1e-4, (ec, ea)
    assert es[0] <= 1e-5, (es, st, c.st_want)


# ---- 1. gradients and statistics over the shape contract ------------------------------------------------------------------------
def check_seeds_and_rejection(shape, NC):
    """CPU only, reference only: every batch size of the shape finds a seed with KAPPA <= KAPPA_MAX within SEEDS_TRIED (and the
    formula of KAPPA's denominator IS the last bias' gradient of float64 autograd); the rejection loop of make_batch keeps its
    'at most half rejected, at most 12 passes' at this shape."""
    D, G, A = shape
    for B in BATCHES:
        c = case(shape, B, NC)
        print("OFFPOLICY_CONTRACT seeds ref {}: kappas tried {}".format(c.what(), ["{:.3g}".format(k) for k in c.kappas]))
        assert c.kappa <= KAPPA_MAX, (shape, B, NC, c.kappas)
        np.testing.assert_allclose(c.bias_grad.numpy(), c.want_a[-1].numpy(), rtol=1e-9, atol=1e-14)
    counts = []
    nets = oc.make_nets(D, G, A, NC, 31)
    b = oc.make_batch(nets, 1024, 32, counts=counts)
    print("OFFPOLICY_CONTRACT rejection ref D={} G={} A={} NC={}: {}".format(D, G, A, NC, counts))
    assert counts[0][0] == 1024 and counts[0][1] <= 512 and len(counts) <= 12
    assert 0.15 <= float(b["done"].float().mean()) <= 0.35


def check_grads(lib, device, shape, B, NC, check="grads"):
    c = case(shape, B, NC)
    assert c.kappa <= KAPPA_MAX, c.kappas
    L = oc.learner(lib, c.nets, device)
    gc_, ga, stats = launch_grads(L, oc.to_device(c.b, device), B, device)
    assert_grads(check, device, c, L, gc_, ga, stats)
    L.close()


# ---- 2. nothing outside the batch is read or written ---------------------------------------------------------------------------
def check_fenced(lib, device, shape, B, NC=2):
    """The case's batch behind NaN fences, `done` at an odd byte, goal words G..3 NaN, y_out inside a sentinel buffer: gradients,
    loss sums, statistics and y bit-equal to the plain call's (itself within section 1's bounds), the sentinels intact."""
    c = case(shape, B, NC)
    G = shape[1]
    L = oc.learner(lib, c.nets, device)
    PA, P = L.actor_params, L.num_params
    y0 = torch.full((B,), oc.SENTINEL, device=device)
    gc0, ga0, st0 = launch_grads(L, oc.to_device(c.b, device), B, device, y=y0)
    assert_grads("fenced", device, c, L, gc0, ga0, st0)
    ey = float((y0.cpu().double() - c.y).abs().max()) / max(float(c.y.abs().max()), 1.0)
    assert ey <= 1e-5, ey
    db, bufs = fenced(c.b, G, device)
    ybuf = torch.full((B + 2 * FENCE,), oc.SENTINEL, device=device)
    gc1, ga1, st1 = launch_grads(L, db, B, device, y=ybuf[FENCE:FENCE + B])
    for name, x, y in (("critic launch", gc0, gc1), ("actor launch", ga0, ga1), ("statistics", st0, st1), ("y", y0, ybuf[FENCE:FENCE + B])):
        assert torch.equal(oc.bits(x), oc.bits(y)), name   # (the other segment's gradient words too: sentinels on both sides)
    assert not torch.isnan(gc1[PA:]).any() and not torch.isnan(ga1[:PA]).any() and not torch.isnan(ga1[P + 1])
    sent = oc.bits(torch.full((FENCE,), oc.SENTINEL))
    assert torch.equal(oc.bits(ybuf[:FENCE]), sent) and torch.equal(oc.bits(ybuf[FENCE + B:]), sent)
    for buf in bufs:   # (the inputs are as they were)
        assert buf.dtype == torch.uint8 or bool(torch.isnan(buf[:FENCE]).all() and torch.isnan(buf[FENCE + B:]).all())
    L.close()


# ---- 3. the tile split and stale slabs ---------------------------------------------------------------------------------------------
def check_tile_split(lib, device, shape, NC=2, small=65):
    """SPLIT_B rows against float64; then `small` rows on the same learner equal a fresh learner's call bit for bit (the slabs of the
    larger call's other 255 workgroups are not summed)."""
    c = case(shape, SPLIT_B, NC)
    L = oc.learner(lib, c.nets, device)
    gc_, ga, stats = launch_grads(L, oc.to_device(c.b, device), SPLIT_B, device)
    assert_grads("tile_split", device, c, L, gc_, ga, stats)
    sb = oc.to_device({k: v[:small].contiguous() for k, v in c.b.items()}, device)
    stale = launch_grads(L, sb, small, device)
    F = oc.learner(lib, c.nets, device)
    fresh = launch_grads(F, sb, small, device)
    for name, x, y in zip(("critic launch", "actor launch", "statistics"), stale, fresh):
        assert torch.equal(oc.bits(x), oc.bits(y)), name
    assert not torch.equal(oc.bits(stale[0]), oc.bits(gc_))
    L.close(), F.close()


# ---- 4. k_ddpg_apply and k_ddpg_polyak against float64 -----------------------------------------------------------------------------
def clip_adam64(p, g, m, v, t, lr, max_norm):
    """clip_grad_norm_(max_norm) + torch.optim.Adam(betas=BETAS, eps=ADAM_EPS) in float64 from the state (p, m, v, t), fed the
    gradient g (test_ppo_hip_contract._clip_adam64 with this file's hyper-parameters).  -> (parameters, m, v, clip coefficient)"""
    p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
    coef = min(max_norm / (float(g.norm()) + 1e-6), 1.0) if max_norm > 0 else 1.0
    g = g * coef
    b1, b2 = BETAS
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    t = t + 1
    p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + ADAM_EPS)
    return p, m, v, coef


def lerp64(t, p, tau):
    t, p = t.detach().cpu().double(), p.detach().cpu().double()
    return t + tau * (p - t)


def state_error(got, want):
    """test_ppo_hip_contract._check_state's closeness (parameters rtol 1e-6 + 1e-7; both moments rtol 1e-6 with a floor of 1e-6 of
    the moment vector's largest entry) as the worst |x - want| / tolerance over (parameters, m, v): <= 1 passes."""
    worst = 0.0
    for i, (x, w) in enumerate(zip(got, want)):
        x, w = x.detach().cpu().double(), w.detach().cpu().double()
        atol = 1e-7 if i == 0 else 1e-6 * float(w.abs().max())
        worst = max(worst, float(((x - w).abs() / (atol + 1e-6 * w.abs())).max()))
    return worst


SEGMENTS = {nat.DDPG_CRITICS: ("critics", LR_CRITIC, MAXN_CRITIC), nat.DDPG_ACTOR: ("actor", LR_ACTOR, MAXN_ACTOR)}


def check_apply64(lib, device):
    """Three steps per segment from the counters STEPS0 and nonzero moments, gradients of norm 2, 0.2 and 0.01 (the actor's clip norm is
    0.05, the critics' 0.5: the middle one is clipped for the actor only), each against float64 clip + Adam from the learner's own
    state; the other segment bit-equal; acc[4] accumulates; then the Polyak pass at tau 0.3, 0.5 and 0.7 against the float64 lerp
    (rtol 1e-6 with offpolicy_common.check_apply's floor of 1e-7 for entries that cancel)."""
    nets = oc.make_nets(27, 2, 4, 2, 5)
    L = oc.learner(lib, nets, device)
    set_hparams(L)
    PA, P = L.actor_params, L.num_params
    gen = torch.Generator().manual_seed(9)
    L.steps.copy_(torch.tensor(STEPS0, dtype=torch.int32))
    L.exp_avg.copy_((0.01 * torch.randn(P, generator=gen)).to(device))
    L.exp_avg_sq.copy_(((0.01 * torch.randn(P, generator=gen)) ** 2 + 1e-7).to(device))
    acc0 = [0.5, -0.25, 1.5, -2.0]
    L.stats.copy_(torch.tensor(acc0).to(device))
    acc64 = list(acc0)
    B, worst, worst_acc = 64, 0.0, 0.0
    state = lambda: (L.flat, L.exp_avg, L.exp_avg_sq)
    for seg in (nat.DDPG_CRITICS, nat.DDPG_ACTOR):
        name, lr, maxn = SEGMENTS[seg]
        lo, hi = (PA, P) if seg == nat.DDPG_CRITICS else (0, PA)
        other = slice(0, PA) if seg == nat.DDPG_CRITICS else slice(PA, P)
        before = [oc.bits(t)[other].clone() for t in state()] + [oc.bits(L.steps)[1 - seg].clone(), oc.bits(L.target).clone()]
        for step, norm in enumerate([2.0, 0.2, 0.01]):
            g = torch.randn(hi - lo, generator=gen, dtype=torch.float64)
            g = (g * (norm / float(g.norm()))).float()
            flat = torch.full((P + nat.DDPG_NSTAT,), float("nan"))   # (the other segment's gradient words are never read)
            flat[lo:hi] = g
            sums = torch.tensor([6.5, -13.0, 26.0, -3.25]) * (step + 1)
            flat[P:] = sums
            t0 = int(L.steps[seg].item())
            p, m, v, coef = clip_adam64(L.flat[lo:hi], g, L.exp_avg[lo:hi], L.exp_avg_sq[lo:hi], t0, lr, maxn)
            assert (coef < 1.0) == (norm > maxn), (name, norm, coef)
            L.apply(seg, flat.to(device), B)
            e = state_error([t[lo:hi] for t in state()], (p, m, v))
            worst = max(worst, e)
            assert e <= 1.0, (name, step, e)
            assert int(L.steps[seg].item()) == t0 + 1
            if seg == nat.DDPG_CRITICS:
                for k in (0, 2, 3):
                    acc64[k] += float(sums[k]) / B
            else:
                acc64[1] -= float(sums[1]) / B
            got = L.stats.cpu().double().tolist()
            ea = max(abs(x - w) / abs(w) for x, w in zip(got, acc64))
            worst_acc = max(worst_acc, ea)
            assert ea <= 1e-6, (name, step, got, acc64)
        after = [oc.bits(t)[other] for t in state()] + [oc.bits(L.steps)[1 - seg], oc.bits(L.target)]
        for x, y in zip(before, after):
            assert torch.equal(x, y), name
    assert L.steps.cpu().tolist() == [STEPS0[0] + 3, STEPS0[1] + 3]
    worst_t = 0.0
    zero = torch.zeros(P + nat.DDPG_NSTAT, device=device)
    for tau in (0.3, 0.5, 0.7):
        L.hparams.tau = tau
        t0 = L.target.clone()
        L.apply(nat.DDPG_ACTOR, zero, B, polyak=True)
        want = lerp64(t0, L.flat, tau)
        e = float(((L.target.cpu().double() - want).abs() / (1e-7 + 1e-6 * want.abs())).max())
        worst_t = max(worst_t, e)
        assert e <= 1.0, (tau, e)
        assert not torch.equal(oc.bits(L.target), oc.bits(t0))
    say("apply", device, "D=27 G=2 A=4 NC=2", state_of_tol=worst, acc_rel=worst_acc, polyak_of_tol=worst_t)
    L.close()


# ---- 5. fwg_ddpg_step equals its halves --------------------------------------------------------------------------------------------
def step(L, db, B, u, delay):
    """fwg_ddpg_step on the learner's own state (HipDDPG.update without the zeroing of the statistics and the host read)."""
    p = lambda t: ctypes.c_void_p(int(t.data_ptr()))
    bs = L.batch_struct(db)
    nat.check(L._lib, L._lib.fwg_ddpg_step(L._h, ctypes.byref(bs), B, u, delay, ctypes.byref(L.hparams), p(L.flat), p(L.target), p(L.exp_avg),
                                           p(L.exp_avg_sq), p(L.steps), p(L.stats), L._stream()))


def halves(L, db, B, u, delay):
    bs = L.batch_struct(db)
    L.critic_grad(bs, B, L.grad)
    L.apply(nat.DDPG_CRITICS, L.grad, B)
    if u % delay == 0:
        L.actor_grad(bs, B, L.grad)
        L.apply(nat.DDPG_ACTOR, L.grad, B, polyak=True)


STATE = ("flat", "target", "exp_avg", "exp_avg_sq", "steps", "stats")


def assert_same_state(L, T, msg):
    for name in STATE:
        assert torch.equal(oc.bits(getattr(L, name)), oc.bits(getattr(T, name))), (msg, name)


def check_step_equals_halves(lib, device, shape=(27, 2, 4), NC=2, B=65):
    c = case(shape, B, NC)
    batches = [oc.to_device(b, device) for b in (c.b, oc.make_batch(c.nets, B, c.seed + 7))]
    for delay in (1, 2):
        L, T = oc.learner(lib, c.nets, device), oc.learner(lib, c.nets, device)
        set_hparams(L), set_hparams(T)
        PA = L.actor_params
        for u in range(1, delay + 1):
            snap = {name: oc.bits(getattr(T, name)).clone() for name in STATE}
            halves(L, batches[u - 1], B, u, delay)
            step(T, batches[u - 1], B, u, delay)
            assert_same_state(L, T, (delay, u))
            now = {name: oc.bits(getattr(T, name)) for name in STATE}
            for name in ("flat", "exp_avg", "exp_avg_sq"):   # the critics move on every update
                assert not torch.equal(now[name][PA:], snap[name][PA:]), (delay, u, name)
            assert int(now["steps"][1]) == u
            moved = u % delay == 0
            for name in ("flat", "exp_avg", "exp_avg_sq"):
                assert torch.equal(now[name][:PA], snap[name][:PA]) != moved, (delay, u, name)
            assert torch.equal(now["target"], snap["target"]) != moved
            assert torch.equal(now["steps"][0], snap["steps"][0]) != moved and torch.equal(now["stats"][1], snap["stats"][1]) != moved
        L.close(), T.close()
    say("step_halves", device, "D={} G={} A={} B={} NC={}".format(*(shape + (B, NC))), bit_equal=1)


# ---- 6. a whole run against float64 at the learner's own state ---------------------------------------------------------------------
def nets_of(L, shape, NC):
    """CPU modules holding the learner's online and target parameters."""
    D, G, A = shape
    nets = [GoalActor(D, G, A), [GoalCritic(D, G, A) for _ in range(NC)], GoalActor(D, G, A), [GoalCritic(D, G, A) for _ in range(NC)]]
    with torch.no_grad():
        for mods, src in (([nets[0]] + nets[1], L.flat.cpu()), ([nets[2]] + nets[3], L.target.cpu())):
            o = 0
            for m in mods:
                for p in m.parameters():
                    p.copy_(src[o:o + p.numel()].view_as(p))
                    o += p.numel()
    return nets


def relu_margin(nets, b):
    """The smallest |ReLU pre-activation| of Q_0(o, g, pi(o, g)) in float64."""
    actor, c0 = copy.deepcopy(nets[0]).double(), copy.deepcopy(nets[1][0]).double()
    G = actor.goal_dim
    o, g = b["observation"].double(), b["desired_rows"][:, :G].double()
    with torch.no_grad():
        z1, z2, _ = oc._preacts(c0.net, torch.cat([o, g, actor(o, g)], 1))
    return min(float(z1.abs().min()), float(z2.abs().min()))


def check_run64(lib, device, shape=(27, 2, 4), NC=2, B=129, delay=2, updates=6):
    """`updates` updates with section 4's hyper-parameters.  Every half of every update starts from the learner's own state: the
    batch is drawn (offpolicy_common's rejection) against the parameters the learner holds before the update, the half's gradient is
    held to float64 autograd at those parameters (1e-4 relative Frobenius error), and the state behind the half to float64 clip +
    Adam from the learner's own parameters, moments and counter fed the learner's gradient (state_error), the target to the float64
    lerp: test_ppo_hip_contract._check_update's two stages, which between them hold every word of the new state to float64.
    (One stage -- float64 clip + Adam fed the float64 GRADIENT, under state_error -- cannot hold and is printed, not asserted: a
    gradient that is within 1e-4, here 1e-5, of float64 moves the first moment by 1e-5 of itself, ten times the 1e-6 that
    state_error grants a moment.  Measured: up to 4.43 x the tolerance on the host emulation and 4.40 x on the MI355X, both at the
    second update's actor step, with the gradients at 4e-6 .. 7e-6 of float64.)
    A twin learner's fwg_ddpg_step stays bit-equal to the halves throughout.  The actor half runs behind the critics' step,
    which moves the ReLU pre-activations of Q_0(o, g, pi) the rejection saw: the margin that is left, from the reference, is
    asserted as a cap on the inputs (>= 1e-5; fp32 and float64 differ by ~1e-6 there)."""
    D, G, A = shape
    nets = oc.make_nets(D, G, A, NC, 61)
    L, T = oc.learner(lib, nets, device), oc.learner(lib, nets, device)
    set_hparams(L), set_hparams(T)
    PA, P = L.actor_params, L.num_params
    names_a, names_c = names_of(L)
    worst_g, worst_s, worst_64, worst_t, margin = 0.0, 0.0, 0.0, 0.0, float("inf")
    for u in range(1, updates + 1):
        now = nets_of(L, shape, NC)
        b = oc.make_batch(now, B, 62 + u)
        db = oc.to_device(b, device)
        bs = L.batch_struct(db)
        for seg in ((nat.DDPG_CRITICS, nat.DDPG_ACTOR) if u % delay == 0 else (nat.DDPG_CRITICS,)):
            name, lr, maxn = SEGMENTS[seg]
            lo, hi = (PA, P) if seg == nat.DDPG_CRITICS else (0, PA)
            if seg == nat.DDPG_ACTOR:
                now = nets_of(L, shape, NC)   # (the critics as just updated)
                margin = min(margin, relu_margin(now, b))
            want_c, want_a, _, _, _ = oc.ref_grads(now, b)
            want = want_c if seg == nat.DDPG_CRITICS else want_a
            t0, tgt0 = int(L.steps[seg].item()), L.target.clone()
            before = [t[lo:hi].clone() for t in (L.flat, L.exp_avg, L.exp_avg_sq)]
            if seg == nat.DDPG_CRITICS:
                L.critic_grad(bs, B, L.grad)
            else:
                L.actor_grad(bs, B, L.grad)
            eg = frobenius(L.grad[lo:hi], names_c if seg == nat.DDPG_CRITICS else names_a, want)
            p, m, v, _ = clip_adam64(before[0], L.grad[lo:hi], before[1], before[2], t0, lr, maxn)
            L.apply(seg, L.grad, B, polyak=seg == nat.DDPG_ACTOR)
            got = [t[lo:hi] for t in (L.flat, L.exp_avg, L.exp_avg_sq)]
            es = state_error(got, (p, m, v))
            e64 = state_error(got, clip_adam64(before[0], torch.cat([x.reshape(-1) for x in want]), before[1], before[2], t0, lr, maxn)[:3])
            worst_g, worst_s, worst_64 = max(worst_g, eg[0]), max(worst_s, es), max(worst_64, e64)
            print("  update {} {}: gradient {:.3e} ({}), state / tolerance {:.3f} (fed the float64 gradient: {:.3f})".format(u, name, eg[0], eg[1], es, e64))
            assert eg[0] <= 1e-4, (u, name, eg)
            assert es <= 1.0, (u, name, es)
            assert int(L.steps[seg].item()) == t0 + 1
            if seg == nat.DDPG_ACTOR:
                w = lerp64(tgt0, L.flat, L.hparams.tau)
                et = float(((L.target.cpu().double() - w).abs() / (1e-7 + 1e-6 * w.abs())).max())
                worst_t = max(worst_t, et)
                assert et <= 1.0, (u, et)
        step(T, db, B, u, delay)
        assert_same_state(L, T, u)
    say("run", device, "D={} G={} A={} B={} NC={} delay={} updates={}".format(D, G, A, B, NC, delay, updates), frobenius=worst_g,
        state_of_tol=worst_s, polyak_of_tol=worst_t, relu_margin=margin, state_fed_float64_gradient_of_tol=worst_64)
    assert margin >= 1e-5, margin
    assert L.steps.cpu().tolist() == [updates // delay, updates]
    L.close(), T.close()


# ---- 7. captured equals eager (GPU only) -------------------------------------------------------------------------------------------
def check_captured_equals_eager(lib, device, shape=(27, 2, 4), NC=2, B=129):
    """One fwg_ddpg_step (policy_delay 1) captured after an eager warm-up on copies of the state, the static batch refilled and the
    graph replayed three times: the state bit-equal to three eager steps of a second learner."""
    c = case(shape, B, NC)
    batches = [c.b] + [oc.make_batch(c.nets, B, c.seed + 10 + i) for i in range(2)]
    G_, E = oc.learner(lib, c.nets, device), oc.learner(lib, c.nets, device)
    set_hparams(G_), set_hparams(E)
    static = {k: v.clone() for k, v in oc.to_device(batches[0], device).items()}
    saved = {name: getattr(G_, name).clone() for name in STATE}
    step(G_, static, B, 1, 1)   # the warm-up; then the state goes back IN PLACE (the capture holds these pointers)
    torch.cuda.synchronize(device)
    for name in STATE:
        getattr(G_, name).copy_(saved[name])
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(G_, static, B, 1, 1)
    assert_same_state(G_, E, "the capture ran nothing")
    for i, b in enumerate(batches):
        for k, v in b.items():
            static[k].copy_(v.to(device))
        graph.replay()
        step(E, oc.to_device(b, device), B, i + 1, 1)
    torch.cuda.synchronize(device)
    assert_same_state(G_, E, "after three replays")
    assert G_.steps.cpu().tolist() == [3, 3]
    say("captured", device, "D={} G={} A={} B={} NC={}".format(*(shape + (B, NC))), bit_equal=1)
    del graph
    G_.close(), E.close()
