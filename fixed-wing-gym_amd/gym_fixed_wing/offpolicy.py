"""DDPG -- the off-policy learner behind replay.HindsightReplay: DDPG, or with n_critics=2 / policy_delay=2 TD3's clipped double-Q
and delayed actor step (without TD3's target-policy smoothing noise), on goal-conditioned 64-64 ReLU networks.

    agent = DDPG(vec.obs_dim, env.spec.n, update="hip")
    a = agent.act(obs, desired_goal, noise=0.2)
    stats = agent.update(replay.sample(4096))      # {"critic_loss", "actor_loss", "q_mean", "target_mean"}

Update u (counting from 1) on a minibatch (o, o', a, g, r, done):
    a' = pi_target(o', g);  y = r + gamma (1 - done) min_j Q_target,j(o', g, a');  L_c = sum_j mean (Q_j(o, g, a) - y)^2;  Adam on the critics
    if u % policy_delay == 0:  L_a = -mean Q_0(o, g, pi(o, g)) with the critics as just updated;  Adam on the actor;
                               theta_target <- lerp(theta_target, theta, tau) on everything
Two updaters behind one interface, as learner.py's: TorchDDPGUpdater (autograd, torch.optim.Adam, lerp_) and HipDDPG (the kernels of
csrc/fwgym_offpolicy.h; include/fwgym.h "Off-policy update").  HipDDPG keeps the online and the target parameters as two flat float32
buffers in the layout actor | critic 0 | critic 1; the modules' parameters are VIEWS of the online buffer, so act() sees the updated
weights with no copy.  An update is a handful of eager launches (HindsightReplay.sample's `serial` travels by value: no graph)."""
import ctypes

import numpy as np
import torch
from torch import nn

from . import _native as nat

STAT_KEYS = ("critic_loss", "actor_loss", "q_mean", "target_mean")
_BATCH_KEYS = ("observation", "next_observation", "action", "desired_rows", "reward", "done")
GOAL_STRIDE = 4   # words of a goal row (HindsightReplay.sample's "desired_rows")
MAX_WIDTH = 64    # the HIP path's limit on obs_dim + goal_dim + act_dim: one LDS tile row


def _mlp(n_in, n_out, tanh):
    layers = [nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)]
    return nn.Sequential(*(layers + ([nn.Tanh()] if tanh else [])))


class GoalActor(nn.Module):
    """pi(o, g) = tanh(W3 relu(W2 relu(W1 [o | g] + b1) + b2) + b3)."""

    def __init__(self, obs_dim, goal_dim, act_dim):
        super().__init__()
        self.obs_dim, self.goal_dim, self.act_dim = int(obs_dim), int(goal_dim), int(act_dim)
        self.net = _mlp(self.obs_dim + self.goal_dim, self.act_dim, True)

    def forward(self, obs, goal):
        return self.net(torch.cat([obs, goal], dim=1))


class GoalCritic(nn.Module):
    """Q(o, g, a) = w3 relu(W2 relu(W1 [o | g | a] + b1) + b2) + b3, one value per row."""

    def __init__(self, obs_dim, goal_dim, act_dim):
        super().__init__()
        self.obs_dim, self.goal_dim, self.act_dim = int(obs_dim), int(goal_dim), int(act_dim)
        self.net = _mlp(self.obs_dim + self.goal_dim + self.act_dim, 1, False)

    def forward(self, obs, goal, action):
        return self.net(torch.cat([obs, goal, action], dim=1)).squeeze(1)


def ddpg_critic_loss(critics, actor_target, critics_target, obs, next_obs, action, goal, reward, done, gamma):
    """(L_c, y, [Q_j(o, g, a)]): the TD target y = r + gamma (1 - done) min_j Q_target,j(o', g, pi_target(o', g)) -- no gradient
    flows through it; a terminal sample's next observation is the next episode's, masked by `done` -- and L_c = sum_j mean (Q_j - y)^2."""
    with torch.no_grad():
        a2 = actor_target(next_obs, goal)
        q2 = critics_target[0](next_obs, goal, a2)
        for c in critics_target[1:]:
            q2 = torch.min(q2, c(next_obs, goal, a2))
        y = reward + gamma * (1.0 - done) * q2
    qs = [c(obs, goal, action) for c in critics]
    return sum(((q - y) ** 2).mean() for q in qs), y, qs


def ddpg_actor_loss(actor, critic, obs, goal):
    """L_a = -mean Q_0(o, g, pi(o, g)); its gradient is taken for the actor's parameters only."""
    return -critic(obs, goal, actor(obs, goal)).mean()


def ddpg_losses(actor, critics, actor_target, critics_target, obs, next_obs, action, goal, reward, done, gamma):
    """(L_c, L_a, stats) of one minibatch, the torch statement of the update's two losses (ddpg_critic_loss, ddpg_actor_loss -- the
    functions TorchDDPGUpdater steps on, so yardstick and torch path are one text): `critics` / `critics_target` are lists of 1 or 2
    GoalCritic, `done` is 0 / 1 in the dtype of the rest.  L_c's gradient is taken for the critics' parameters and L_a's for the
    actor's only."""
    critic_loss, y, qs = ddpg_critic_loss(critics, actor_target, critics_target, obs, next_obs, action, goal, reward, done, gamma)
    actor_loss = ddpg_actor_loss(actor, critics[0], obs, goal)
    stats = {"critic_loss": critic_loss.detach(), "actor_loss": actor_loss.detach(), "q_mean": qs[0].detach().mean(), "target_mean": y.mean()}
    return critic_loss, actor_loss, stats


def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))


def _check_batch(batch, obs_dim, act_dim, device):
    """The minibatch as HindsightReplay.sample returns it -> {key: tensor}; a refusal names the entry."""
    out = {}
    for k in _BATCH_KEYS:
        if k not in batch:
            raise ValueError("DDPG.update: the batch has no '{}' (a dict as HindsightReplay.sample returns it)".format(k))
        out[k] = _as_tensor(batch[k])
    B = int(out["observation"].shape[0]) if out["observation"].dim() == 2 else -1
    want = {"observation": (B, obs_dim), "next_observation": (B, obs_dim), "action": (B, act_dim), "desired_rows": (B, GOAL_STRIDE),
            "reward": (B,), "done": (B,)}
    for k in _BATCH_KEYS:
        t = out[k]
        if B < 1 or tuple(t.shape) != want[k]:
            raise ValueError("DDPG.update: batch['{}'] has shape {}, this learner (obs_dim {}, act_dim {}) needs {}".format(
                k, tuple(t.shape), obs_dim, act_dim, tuple("B" if i == 0 else s for i, s in enumerate(want[k]))))
        if t.dtype != (torch.uint8 if k == "done" else torch.float32) or not t.is_contiguous():
            raise ValueError("DDPG.update: batch['{}'] must be a contiguous {} tensor".format(k, "uint8" if k == "done" else "float32"))
        if t.device.type != torch.device(device).type:
            raise ValueError("DDPG.update: batch['{}'] is on {}, the learner on {}".format(k, t.device, device))
    return out, B


def _flat(modules):
    return torch.cat([p.detach().reshape(-1) for m in modules for p in m.parameters()])


class TorchDDPGUpdater(object):
    """The update through torch autograd, torch.optim.Adam and lerp_ (examples/train_her.py's loop body at policy_delay 1, one critic)."""

    def __init__(self, actor, critics, gamma, tau, lr_actor, lr_critic, policy_delay, max_grad_norm, device):
        import copy
        self.actor, self.critics, self.device = actor, critics, torch.device(device)
        self.actor_t, self.critics_t = copy.deepcopy(actor), [copy.deepcopy(c) for c in critics]
        self.gamma, self.tau, self.policy_delay, self.max_grad_norm = gamma, tau, policy_delay, max_grad_norm
        self.opt_a = torch.optim.Adam(actor.parameters(), lr=lr_actor)
        self.opt_c = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=lr_critic)
        self._last_actor_loss = 0.0

    def params(self):
        return _flat([self.actor] + self.critics)

    def target_params(self):
        return _flat([self.actor_t] + self.critics_t)

    def load_params(self, flat, target):
        with torch.no_grad():
            for mods, src in (([self.actor] + self.critics, flat), ([self.actor_t] + self.critics_t, target)):
                o = 0
                for m in mods:
                    for p in m.parameters():
                        p.copy_(src[o:o + p.numel()].view_as(p))
                        o += p.numel()

    def update(self, b, B, u):
        G = self.actor.goal_dim
        o, o2, a, g, r = b["observation"], b["next_observation"], b["action"], b["desired_rows"][:, :G], b["reward"]
        done = b["done"].float()
        critic_loss, y, qs = ddpg_critic_loss(self.critics, self.actor_t, self.critics_t, o, o2, a, g, r, done, self.gamma)
        st ={"critic_loss": critic_loss.detach(), "q_mean": qs[0].detach().mean(), "target_mean": y.mean()}
        self.opt_c.zero_grad()
        critic_loss.backward()
        if self.max_grad_norm is not None:
            nn.utils.clip_grad_norm_(self.opt_c.param_groups[0]["params"], self.max_grad_norm)
        self.opt_c.step()
        if u % self.policy_delay == 0:
            actor_loss = ddpg_actor_loss(self.actor, self.critics[0], o, g)
            self.opt_a.zero_grad()
            actor_loss.backward()   # (the critic's gradients it leaves are zeroed before the next critic step)
            if self.max_grad_norm is not None:
                nn.utils.clip_grad_norm_(self.actor.parameters(), self.max_grad_norm)
            self.opt_a.step()
            with torch.no_grad():
                for net, tgt in zip([self.actor] + self.critics, [self.actor_t] + self.critics_t):
                    for p, pt in zip(net.parameters(), tgt.parameters()):
                        pt.lerp_(p, self.tau)
            self._last_actor_loss = float(actor_loss.detach())
        return {"critic_loss": float(st["critic_loss"]), "actor_loss": self._last_actor_loss, "q_mean": float(st["q_mean"]),
                "target_mean": float(st["target_mean"])}


class HipDDPG(object):
    """The update as HIP kernels through `lib`.  flat / target: the online and target parameters; exp_avg / exp_avg_sq: Adam's
    moments (one layout); steps: int32 [2], the actor's and the critics' step counters; grad: a gradient buffer for the halves."""

    def __init__(self, lib, actor, critics, gamma, tau, lr_actor, lr_critic, policy_delay, max_grad_norm, device, betas=(0.9, 0.999), eps=1e-8):
        self._lib, self.actor, self.critics, self.device = lib, actor, critics, torch.device(device)
        D, G, A = actor.obs_dim, actor.goal_dim, actor.act_dim
        if D + G + A > MAX_WIDTH:
            raise ValueError("DDPG(update='hip'): obs_dim + goal_dim + act_dim = {} exceeds {} (obs_dim {}, goal_dim {}, act_dim {}): "
                             "one LDS tile row holds a critic's input".format(D + G + A, MAX_WIDTH, D, G, A))
        self._h = None
        h = ctypes.c_void_p()
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                nat.check(lib, lib.fwg_offpolicy_create(D, G, A, len(critics), ctypes.byref(h)))
        else:
            nat.check(lib, lib.fwg_offpolicy_create(D, G, A, len(critics), ctypes.byref(h)))
        self._h = h
        params = [p for m in [actor] + critics for p in m.parameters()]
        self.num_params, self.actor_params = int(lib.fwg_offpolicy_num_params(h)), int(lib.fwg_offpolicy_actor_params(h))
        if self.num_params != sum(p.numel() for p in params):
            raise ValueError("the networks have {} parameters, the learner's layout {}".format(sum(p.numel() for p in params), self.num_params))
        with torch.no_grad():
            self.flat = torch.cat([p.detach().reshape(-1).float() for p in params]).to(self.device).contiguous()
            o = 0
            for p in params:   # the modules' parameters become views of the flat buffer
                p.data = self.flat[o:o + p.numel()].view_as(p)
                o += p.numel()
        self.target = self.flat.clone()
        z = lambda *s, **k: torch.zeros(*s, device=self.device, **k)
        self.exp_avg, self.exp_avg_sq = z(self.num_params), z(self.num_params)
        self.steps = z(2, dtype=torch.int32)
        self.stats = z(len(STAT_KEYS))
        self.grad = z(self.num_params + nat.DDPG_NSTAT)
        self.policy_delay = policy_delay
        self.hparams = nat.DdpgHparams(gamma, tau, lr_actor, lr_critic, betas[0], betas[1], eps,
                                       *((0.0, 0.0) if max_grad_norm is None else (max_grad_norm, max_grad_norm)))
        self._last_actor_loss = 0.0

    def close(self):
        """Gives the learner's device buffers back NOW.  A learner left to the garbage collector frees them whenever that runs --
        a hipFree in the middle of somebody's graph capture invalidates the capture -- so long-lived processes that capture
        graphs close their learners."""
        if self._h:
            self._lib.fwg_offpolicy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        if self.device.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return ctypes.c_void_p()

    def params(self):
        return self.flat.clone()

    def target_params(self):
        return self.target.clone()

    def load_params(self, flat, target):
        self.flat.copy_(flat)
        self.target.copy_(target)

    @staticmethod
    def batch_struct(b):
        s = nat.OffpolicyBatch()
        s.obs, s.next_obs, s.action = int(b["observation"].data_ptr()), int(b["next_observation"].data_ptr()), int(b["action"].data_ptr())
        s.goal_rows, s.reward, s.done = int(b["desired_rows"].data_ptr()), int(b["reward"].data_ptr()), int(b["done"].data_ptr())
        return s

    # ---- the halves (device pointers; nothing synchronises)
    def critic_grad(self, bs, B, out, td_target=None, params=None, target=None):
        p = lambda t: ctypes.c_void_p(int(t.data_ptr()))
        nat.check(self._lib, self._lib.fwg_ddpg_critic_grad(self._h, ctypes.byref(bs), B, ctypes.byref(self.hparams), p(self.flat if params is None else params),
                                                            p(self.target if target is None else target), p(out),
                                                            ctypes.c_void_p() if td_target is None else p(td_target), self._stream()))

    def actor_grad(self, bs, B, out, params=None):
        p = lambda t: ctypes.c_void_p(int(t.data_ptr()))
        nat.check(self._lib, self._lib.fwg_ddpg_actor_grad(self._h, ctypes.byref(bs), B, p(self.flat if params is None else params), p(out), self._stream()))

    def apply(self, segment, grad, B, polyak=False, params=None, m=None, v=None, steps=None, stats=None, target=None):
        p = lambda t: ctypes.c_void_p(int(t.data_ptr()))
        tgt = self.target if target is None else target
        nat.check(self._lib, self._lib.fwg_ddpg_apply(self._h, segment, p(grad), B, ctypes.byref(self.hparams), p(self.flat if params is None else params),
                                                      p(self.exp_avg if m is None else m), p(self.exp_avg_sq if v is None else v),
                                                      p(self.steps if steps is None else steps), p(self.stats if stats is None else stats),
                                                      p(tgt) if polyak else ctypes.c_void_p(), self._stream()))

    def update(self, b, B, u):
        p = lambda t: ctypes.c_void_p(int(t.data_ptr()))
        self.stats.zero_()
        bs = self.batch_struct(b)
        nat.check(self._lib, self._lib.fwg_ddpg_step(self._h, ctypes.byref(bs), B, u, self.policy_delay, ctypes.byref(self.hparams), p(self.flat),
                                                     p(self.target), p(self.exp_avg), p(self.exp_avg_sq), p(self.steps), p(self.stats), self._stream()))
        st = dict(zip(STAT_KEYS, self.stats.tolist()))
        if u % self.policy_delay == 0:
            self._last_actor_loss = st["actor_loss"]
        st["actor_loss"] = self._last_actor_loss
        return st


class DDPG(object):
    """DDPG / TD3-style learner on goal-conditioned 64-64 ReLU networks.  update: "torch" or "hip" (obs_dim + goal_dim + act_dim
    <= 64).  max_grad_norm: clip_grad_norm_ per SEGMENT before its Adam step -- the actor's gradient by its own norm, and the critics'
    by ONE joint norm over both critics, as they are one optimiser's parameters (None: no clipping).  seed: seeds torch
    before the networks are made.  On an update without an actor step (u % policy_delay != 0) `actor_loss` repeats the last one."""

    def __init__(self, obs_dim, goal_dim, act_dim=3, n_critics=1, gamma=0.98, tau=0.05, lr_actor=1e-3, lr_critic=1e-3, policy_delay=1,
                 max_grad_norm=None, update="torch", device=None, seed=None, _lib=None):
        if update not in ("torch", "hip"):
            raise ValueError("DDPG: update must be 'torch' or 'hip', it is {!r}".format(update))
        if n_critics not in (1, 2):
            raise ValueError("DDPG: n_critics must be 1 or 2, it is {!r}".format(n_critics))
        if int(policy_delay) != policy_delay or policy_delay < 1:
            raise ValueError("DDPG: policy_delay must be a positive integer, it is {!r}".format(policy_delay))
        if int(obs_dim) < 1 or not 1 <= int(goal_dim) <= GOAL_STRIDE or not 1 <= int(act_dim) <= 4:
            raise ValueError("DDPG: obs_dim must be positive, goal_dim and act_dim in 1 .. 4 (obs_dim {}, goal_dim {}, act_dim {})".format(
                obs_dim, goal_dim, act_dim))
        if device is None:
            device = "cuda:0" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.obs_dim, self.goal_dim, self.act_dim, self.n_critics = int(obs_dim), int(goal_dim), int(act_dim), int(n_critics)
        self.update_path, self.updates = update, 0
        if seed is not None:
            torch.manual_seed(seed)
        self.actor = GoalActor(obs_dim, goal_dim, act_dim).to(self.device)
        self.critics = [GoalCritic(obs_dim, goal_dim, act_dim).to(self.device) for _ in range(self.n_critics)]
        args = (float(gamma), float(tau), float(lr_actor), float(lr_critic), int(policy_delay), None if max_grad_norm is None else float(max_grad_norm),
                self.device)
        if update == "hip":   # (no fall-back: a missing library or kernel is an error)
            self.updater = HipDDPG(_lib if _lib is not None else nat.load_library(), self.actor, self.critics, *args)
        else:
            self.updater = TorchDDPGUpdater(self.actor, self.critics, *args)

    def act(self, obs, goal, noise=0.0):
        """pi(obs, goal), with Gaussian exploration noise of std `noise` clipped to [-1, 1]."""
        with torch.no_grad():
            a = self.actor(obs, goal)
            if noise > 0.0:
                a = (a + noise * torch.randn_like(a)).clamp(-1.0, 1.0)
        return a

    def update(self, batch):
        """One update on a minibatch dict exactly as HindsightReplay.sample returns it -> {"critic_loss", "actor_loss", "q_mean",
        "target_mean"} (floats: this call waits for the update)."""
        b, B = _check_batch(batch, self.obs_dim, self.act_dim, self.device)
        stats = self.updater.update(b, B, self.updates + 1)
        self.updates += 1   # (behind the update: a refused call leaves the policy-delay counter where it was)
        return stats

    def close(self):
        """Releases the HIP learner's device buffers (HipDDPG.close); the torch path holds nothing to release."""
        if hasattr(self.updater, "close"):
            self.updater.close()

    def save(self, path):
        np.savez(path, params=self.updater.params().cpu().numpy(), target=self.updater.target_params().cpu().numpy(),
                 dims=np.array([self.obs_dim, self.goal_dim, self.act_dim, self.n_critics]), updates=np.array(self.updates))

    def load(self, path):
        """Weights (online and target) and the update counter; Adam's moments start afresh."""
        with np.load(path) as z:
            if [int(x) for x in z["dims"]] != [self.obs_dim, self.goal_dim, self.act_dim, self.n_critics]:
                raise ValueError("DDPG.load: {} holds networks of (obs_dim, goal_dim, act_dim, n_critics) = {}, this learner {}".format(
                    path, [int(x) for x in z["dims"]], [self.obs_dim, self.goal_dim, self.act_dim, self.n_critics]))
            self.updater.load_params(torch.as_tensor(z["params"], device=self.device), torch.as_tensor(z["target"], device=self.device))
            self.updates = int(z["updates"])
