"""The two PPO updaters behind PPO(update="torch" | "hip" | "hip_cnn"): stable-baselines PPO2's minibatch step -- loss, backward,
clip_grad_norm_, Adam -- by torch autograd (TorchUpdater) or as HIP kernels (HipLearner; include/fwgym.h "PPO update").  Both have
update(batch, perms, mb, nmb, lr, cliprange, ent_coef, vf_coef, max_grad_norm, world=1, group=None) -> {stat: mean over the steps}:
`perms` yields one permutation of the n rows per epoch (int64, on the device), `lr=None` is the rate in force (the construction-time
one, or the last one given), and the rollout head holds the new weights on return.

HipLearner: the torch MlpPolicy's (or, for a CNN head, CnnMlpPolicy's) parameters live as VIEWS of one flat float32 buffer that the kernels update in place (so
state_dict(), save() / load() and deterministic_policy() see the learner's weights with no copy), and the rollout head is repacked
from that buffer on the device after every update.  On the GPU (world size 1) a whole update -- every epoch's advantage moments,
every minibatch step and the head repack -- is captured once per (batch buffers, minibatch size) into ONE hipGraph, a single linear
chain on one stream, and replayed once per update; the hyper-parameters are read on the device, so update(lr=...) and schedules
need no recapture.  With torch.distributed initialised the steps run eagerly: gradient half -> all-reduce of the flat gradient /
world -> apply half.  TorchUpdater: on the GPU (world size 1, no lr passed) each minibatch step is one replayed hipGraph."""
import ctypes
import math

import torch
from torch import nn

from . import _native as nat

STAT_KEYS = ("pg_loss", "vf_loss", "entropy", "approx_kl", "clip_frac")
_BATCH_KEYS = ("obs", "actions", "values", "logp", "adv", "returns")


def _ptr(t, offset=0):
    return ctypes.c_void_p(int(t.data_ptr()) + offset)


def _graph_key(batch, *rest):   # what a captured graph holds by value: the batch's buffers and the scalars baked into it
    return (tuple(int(batch[k].data_ptr()) for k in _BATCH_KEYS),) + rest


def _all_reduce_mean(flat, world, group):   # data-parallel PPO: one all-reduce of the (tiny) flat gradient per minibatch step
    torch.distributed.all_reduce(flat, group=group)
    flat /= world


class HipLearner(object):
    """PPO update of `policy` for the rollout head `actor` (DeviceActor) through `lib`: an MlpPolicy, or a CnnMlpPolicy when the
    head is a CNN head (fwg_learner_create_cnn: the layout includes the conv; the parameter count below guards it).  `graph`:
    capture the update (GPU only).  `lr`: the rate in force until an update is given one."""

    def __init__(self, lib, actor, policy, device, graph=True, betas=(0.9, 0.999), eps=1e-5, lr=2.5e-4):
        self._lib, self.actor, self.policy, self.device = lib, actor, policy, torch.device(device)
        h = ctypes.c_void_p()
        create = lib.fwg_learner_create_cnn if actor.cnn else lib.fwg_learner_create
        nat.check(lib, create(actor._handle, ctypes.byref(h)))
        self._h = h
        params = list(policy.parameters())
        self.num_params = int(lib.fwg_learner_num_params(h))
        if self.num_params != sum(p.numel() for p in params):
            raise ValueError("policy has {} parameters, the learner's layout {}".format(sum(p.numel() for p in params), self.num_params))
        with torch.no_grad():
            self.flat = torch.cat([p.detach().reshape(-1).float() for p in params]).to(self.device).contiguous()
            o = 0
            for p in params:   # the module's parameters become views of the flat buffer (the policy's parameters() order)
                p.data = self.flat[o:o + p.numel()].view_as(p)
                o += p.numel()
        z = lambda *s, **k: torch.zeros(*s, device=self.device, **k)
        self.exp_avg, self.exp_avg_sq = z(self.num_params), z(self.num_params)
        self.step = z(1, dtype=torch.int32)
        self.stats = z(len(STAT_KEYS))
        self.grad = z(self.num_params + nat.PPO_NSTAT)
        self.hparams = z(8, dtype=torch.float64)   # fwg_ppo_hparams
        self.betas, self.eps, self.lr = tuple(float(b) for b in betas), float(eps), lr
        self._graph_ok = bool(graph) and self.device.type == "cuda"
        self._graph = None

    def __del__(self):
        try:
            if self._h:
                self._lib.fwg_learner_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        if self.device.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return ctypes.c_void_p()

    def set_hparams(self, lr, cliprange, ent_coef, vf_coef, max_grad_norm):
        if lr is not None:   # (a given lr stays in force)
            self.lr = lr
        v = torch.tensor([self.lr, cliprange, ent_coef, vf_coef, max_grad_norm, self.betas[0], self.betas[1], self.eps], dtype=torch.float64)
        self.hparams.copy_(v)

    def pack(self):
        """The head's weights from the flat buffer, on the device (no host round trip)."""
        nat.check(self._lib, self._lib.fwg_actor_pack(self._h, _ptr(self.flat), self._stream()))

    # ---- the three calls of a minibatch step (device pointers; nothing synchronises)
    def _batch_struct(self, batch):
        b = nat.PpoBatch()
        for k in _BATCH_KEYS:
            setattr(b, k, int(batch[k].data_ptr()))
        return b

    def moments(self, batch, perm, mb, nmb, out):
        nat.check(self._lib, self._lib.fwg_ppo_moments(self._h, _ptr(batch["adv"]), _ptr(perm), mb, nmb, _ptr(out), self._stream()))

    def grad_half(self, bs, idx, mb, mom, out, params=None):
        nat.check(self._lib, self._lib.fwg_ppo_grad(self._h, ctypes.byref(bs), idx, mb, mom, _ptr(self.flat if params is None else params),
                                                    _ptr(self.hparams), _ptr(out), self._stream()))

    def apply_half(self, grad, mb, params=None, m=None, v=None, step=None, stats=None):
        nat.check(self._lib, self._lib.fwg_ppo_apply(self._h, _ptr(grad), mb, _ptr(self.hparams), _ptr(self.flat if params is None else params),
                                                     _ptr(self.exp_avg if m is None else m), _ptr(self.exp_avg_sq if v is None else v),
                                                     _ptr(self.step if step is None else step), _ptr(self.stats if stats is None else stats),
                                                     self._stream()))

    def full_step(self, bs, idx, mb, mom):
        nat.check(self._lib, self._lib.fwg_ppo_step(self._h, ctypes.byref(bs), idx, mb, mom, _ptr(self.hparams), _ptr(self.flat),
                                                    _ptr(self.exp_avg), _ptr(self.exp_avg_sq), _ptr(self.step), _ptr(self.stats),
                                                    self._stream()))

    # ---- one update
    def _prepare(self, batch):
        for k in _BATCH_KEYS:
            if batch[k].dtype != torch.float32 or not batch[k].is_contiguous():
                raise ValueError("batch[{!r}] must be a contiguous float32 tensor".format(k))
        return {k: batch[k] for k in _BATCH_KEYS}

    def _run(self, batch, perms, mb, nmb, mom, world=1, group=None):
        bs = self._batch_struct(batch)
        for e, perm in enumerate(perms):
            self.moments(batch, perm, mb, nmb, mom[e])
            for k in range(nmb):
                idx, m = _ptr(perm, 8 * k * mb), _ptr(mom[e], 8 * k)
                if world == 1:
                    self.full_step(bs, idx, mb, m)
                else:   # data-parallel PPO: one all-reduce of the flat gradient (+ loss sums) per minibatch step
                    self.grad_half(bs, idx, mb, m, self.grad)
                    _all_reduce_mean(self.grad, world, group)
                    self.apply_half(self.grad, mb)
        self.pack()

    def _capture(self, batch, key):
        dev = self.device
        n, mb, nmb, nep = key[1:]
        g = {"key": key, "perm": torch.zeros((nep, n), dtype=torch.int64, device=dev), "mom": torch.zeros((nep, nmb, 2), device=dev),
             "batch": batch}
        g["perm"].copy_(torch.arange(n, device=dev).expand(nep, n))
        # every kernel once outside the capture, on scratch copies of the state (code objects loaded before the capture)
        bs = self._batch_struct(batch)
        scratch = [t.clone() for t in (self.flat, self.exp_avg, self.exp_avg_sq, self.step, self.stats)]
        self.moments(batch, g["perm"][0], mb, nmb, g["mom"][0])
        self.grad_half(bs, _ptr(g["perm"][0]), mb, _ptr(g["mom"][0]), self.grad, params=scratch[0])
        self.apply_half(self.grad, mb, *scratch)
        self.pack()
        torch.cuda.synchronize(dev)
        g["graph"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g["graph"]):
            self._run(batch, g["perm"], mb, nmb, g["mom"])
        return g

    def update(self, batch, perms, mb, nmb, lr, cliprange, ent_coef, vf_coef, max_grad_norm, world=1, group=None):
        batch, perms = self._prepare(batch), list(perms)   # (every epoch's permutation first: one replay runs them all)
        n, nep = int(batch["obs"].shape[0]), len(perms)
        self.set_hparams(lr, cliprange, ent_coef, vf_coef, max_grad_norm)
        self.stats.zero_()
        if self._graph_ok and world == 1:
            key = _graph_key(batch, n, mb, nmb, nep)
            if self._graph is None or self._graph["key"] != key:
                self._graph = None
                self._graph = self._capture(batch, key)
            g = self._graph
            for e, p in enumerate(perms):
                g["perm"][e].copy_(p)
            g["graph"].replay()
        else:
            perms = [p.contiguous() for p in perms]
            mom = torch.zeros((nep, nmb, 2), device=self.device)
            self._run(batch, perms, mb, nmb, mom, world, group)
        steps = nep * nmb
        return {k: float(v) / steps for k, v in zip(STAT_KEYS, self.stats.tolist())}


def ppo_loss(policy, obs, actions, old_values, old_logp, adv, returns, cliprange, ent_coef, vf_coef):
    """PPO2's loss on one minibatch (stable-baselines ppo2.py setup_model): advantages normalised per minibatch, clipped
    surrogate, value loss clipped around the old value with the SAME range, Gaussian entropy bonus."""
    adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    mean = policy.pi(obs)
    value = policy.vf(obs).squeeze(-1)
    log_std = policy.log_std
    neglogp = 0.5 * (((actions - mean) / log_std.exp()) ** 2).sum(dim=-1) + 0.5 * math.log(2.0 * math.pi) * actions.shape[-1] + log_std.sum()
    ratio = torch.exp(-old_logp - neglogp)
    pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - cliprange, 1.0 + cliprange)).mean()
    v_clipped = old_values + torch.clamp(value - old_values, -cliprange, cliprange)
    vf_loss = 0.5 * torch.max((value - returns) ** 2, (v_clipped - returns) ** 2).mean()
    entropy = (log_std + 0.5 * math.log(2.0 * math.pi * math.e)).sum()
    loss = pg_loss - ent_coef * entropy + vf_coef * vf_loss
    with torch.no_grad():
        stats = {"pg_loss": pg_loss.detach(), "vf_loss": vf_loss.detach(), "entropy": entropy.detach(),
                 "approx_kl": 0.5 * ((neglogp + old_logp) ** 2).mean(), "clip_frac": ((ratio - 1.0).abs() > cliprange).float().mean()}
    return loss, stats


class TorchUpdater(object):
    """PPO update of `policy` (MlpPolicy or CnnMlpPolicy) for the rollout head `actor` through torch autograd and
    torch.optim.Adam(lr, eps=1e-5).  `graph`: capture the minibatch step (GPU only)."""

    def __init__(self, actor, policy, device, graph=True, lr=2.5e-4):
        self.actor, self.policy, self.device = actor, policy, torch.device(device)
        on_gpu = self.device.type == "cuda"
        # (GPU: the fused, capturable form -- ONE launch for all thirteen parameter tensors inside the captured minibatch step)
        self.opt = torch.optim.Adam(policy.parameters(), lr=lr, eps=1e-5, **({"capturable": True, "fused": True} if on_gpu else {}))
        self._graph_ok, self._graph = bool(graph) and on_gpu, None

    def _step(self, mbatch, cliprange, ent_coef, vf_coef, max_grad_norm, world=1, group=None):
        loss, stats = ppo_loss(self.policy, mbatch["obs"], mbatch["actions"], mbatch["values"], mbatch["logp"], mbatch["adv"],
                               mbatch["returns"], cliprange, ent_coef, vf_coef)
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        if world > 1:
            flat = torch.cat([p.grad.reshape(-1) for p in self.policy.parameters()])
            _all_reduce_mean(flat, world, group)
            o = 0
            for p in self.policy.parameters():
                p.grad.copy_(flat[o:o + p.numel()].view_as(p))
                o += p.numel()
        nn.utils.clip_grad_norm_(self.policy.parameters(), max_grad_norm)
        self.opt.step()
        return torch.stack([stats[k] for k in STAT_KEYS])

    def _capture(self, batch, key):
        """One minibatch step -- gather by index, loss, backward, gradient clipping, Adam -- as ONE hipGraph: the 12-64-64
        networks make it ~60 launches of microseconds each, and issued from Python they cost 1.5 ms per step (99 % of a training
        run at 4 096 envs was the optimiser waiting for its own launches)."""
        dev, mb, coefs = self.device, key[1], key[2:]
        g = {"idx": torch.zeros(mb, dtype=torch.long, device=dev), "acc": torch.zeros(len(STAT_KEYS), device=dev), "src": batch, "key": key}
        snap_p = [p.detach().clone() for p in self.policy.parameters()]
        snap_o = [{k: v.clone() for k, v in st.items() if isinstance(v, torch.Tensor)} for st in self.opt.state.values()]

        # ONE gather per step: the six per-transition arrays side by side in a [n, D + 7] buffer, refreshed once per update
        D = batch["obs"].shape[1]
        g["packed"] = torch.empty((batch["obs"].shape[0], D + 7), device=dev)
        g["pack"] = lambda: torch.cat([batch["obs"], batch["actions"], batch["values"][:, None], batch["logp"][:, None],
                                       batch["adv"][:, None], batch["returns"][:, None]], dim=1, out=g["packed"])
        g["pack"]()

        def body():
            m = g["packed"].index_select(0, g["idx"])
            mbatch = {"obs": m[:, :D], "actions": m[:, D:D + 3], "values": m[:, D + 3], "logp": m[:, D + 4], "adv": m[:, D + 5],
                      "returns": m[:, D + 6]}
            g["acc"].add_(self._step(mbatch, *coefs))

        g["idx"].copy_(torch.arange(mb, device=dev))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        had_state = len(snap_o) > 0
        with torch.no_grad():   # the warm-up steps were real optimiser steps: put weights and moments back IN PLACE
            for p, q in zip(self.policy.parameters(), snap_p):
                p.copy_(q)
            for i, st in enumerate(self.opt.state.values()):
                for k, v in st.items():
                    if isinstance(v, torch.Tensor):
                        v.copy_(snap_o[i][k]) if had_state else v.zero_()
        g["graph"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g["graph"]):
            body()
        g["acc"].zero_()
        return g

    def update(self, batch, perms, mb, nmb, lr, cliprange, ent_coef, vf_coef, max_grad_norm, world=1, group=None):
        if lr is not None:   # (a given lr stays in force)
            for pg in self.opt.param_groups:
                pg["lr"] = lr
        coefs, g = (float(cliprange), ent_coef, vf_coef, max_grad_norm), None
        # (known wart, kept -- ADVICE.md: a replayed step runs with the lr it was captured with, whatever param_groups say by now)
        if self._graph_ok and world == 1 and lr is None:
            key = _graph_key(batch, mb, *coefs)
            if self._graph is None or self._graph["key"] != key:
                self._graph = self._capture(batch, key)
            g = self._graph
            g["pack"]()
            g["acc"].zero_()
        acc, steps = torch.zeros(len(STAT_KEYS), device=self.device) if g is None else g["acc"], 0
        for perm in perms:   # (consumed epoch by epoch: one permutation in use at a time)
            for k in range(nmb):
                idx = perm[k * mb:(k + 1) * mb]
                if g is not None:
                    g["idx"].copy_(idx)
                    g["graph"].replay()
                else:
                    acc += self._step({key_: v[idx] for key_, v in batch.items()}, *coefs, world, group)
            steps += nmb
        self.actor.load_policy(self.policy)
        return {k: float(v) / steps for k, v in zip(STAT_KEYS, acc.tolist())}
