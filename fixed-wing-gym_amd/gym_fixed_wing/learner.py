"""The PPO update as HIP kernels (include/fwgym.h "PPO update"; PPO(update="hip")): stable-baselines PPO2's minibatch step --
loss, backward, clip_grad_norm_, Adam -- on the device, the torch MlpPolicy's parameters living as VIEWS of one flat float32
buffer that the kernels update in place (so state_dict(), save() / load() and deterministic_policy() see the learner's weights
with no copy), and the rollout head repacked from that buffer on the device after every update.

On the GPU (world size 1) a whole update -- every epoch's advantage moments, every minibatch step and the head repack -- is
captured once per (batch buffers, minibatch size) into ONE hipGraph, a single linear chain on one stream, and replayed once per
update; the hyper-parameters are read on the device, so update(lr=...) and schedules need no recapture.  With torch.distributed
initialised the steps run eagerly: gradient half -> all-reduce of the flat gradient / world -> apply half."""
import ctypes

import torch

from . import _native as nat

STAT_KEYS = ("pg_loss", "vf_loss", "entropy", "approx_kl", "clip_frac")
_BATCH_KEYS = ("obs", "actions", "values", "logp", "adv", "returns")


def _ptr(t, offset=0):
    return ctypes.c_void_p(int(t.data_ptr()) + offset)


class HipLearner(object):
    """PPO update of `policy` (MlpPolicy) for the rollout head `actor` (DeviceActor) through `lib`.  `graph`: capture the update
    (GPU only)."""

    def __init__(self, lib, actor, policy, device, graph=True, betas=(0.9, 0.999), eps=1e-5):
        self._lib, self.actor, self.policy, self.device = lib, actor, policy, torch.device(device)
        h = ctypes.c_void_p()
        nat.check(lib, lib.fwg_learner_create(actor._handle, ctypes.byref(h)))
        self._h = h
        params = list(policy.parameters())
        self.num_params = int(lib.fwg_learner_num_params(h))
        if self.num_params != sum(p.numel() for p in params):
            raise ValueError("policy has {} parameters, the learner's layout {}".format(sum(p.numel() for p in params), self.num_params))
        with torch.no_grad():
            self.flat = torch.cat([p.detach().reshape(-1).float() for p in params]).to(self.device).contiguous()
            o = 0
            for p in params:   # the module's parameters become views of the flat buffer (MlpPolicy.parameters() order)
                p.data = self.flat[o:o + p.numel()].view_as(p)
                o += p.numel()
        z = lambda *s, **k: torch.zeros(*s, device=self.device, **k)
        self.exp_avg, self.exp_avg_sq = z(self.num_params), z(self.num_params)
        self.step = z(1, dtype=torch.int32)
        self.stats = z(len(STAT_KEYS))
        self.grad = z(self.num_params + nat.PPO_NSTAT)
        self.hparams = z(8, dtype=torch.float64)   # fwg_ppo_hparams
        self.betas, self.eps = tuple(float(b) for b in betas), float(eps)
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
        v = torch.tensor([lr, cliprange, ent_coef, vf_coef, max_grad_norm, self.betas[0], self.betas[1], self.eps], dtype=torch.float64)
        self.hparams.copy_(v)

    def pack(self):
        """The head's weights from the flat buffer, on the device (no host round trip)."""
        nat.check(self._lib, self._lib.fwg_actor_pack(self._h, _ptr(self.flat), self._stream()))

    # ---- the three calls of a minibatch step (device pointers; nothing synchronises)
    def _batch_struct(self, batch):
        b = nat.PpoBatch()
        for f, k in zip(("obs", "actions", "values", "logp", "adv", "returns"), _BATCH_KEYS):
            setattr(b, f, int(batch[k].data_ptr()))
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
        out = {}
        for k in _BATCH_KEYS:
            t = batch[k]
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("batch[{!r}] must be a contiguous float32 tensor".format(k))
            out[k] = t
        return out

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
                    torch.distributed.all_reduce(self.grad, group=group)
                    self.grad /= world
                    self.apply_half(self.grad, mb)
        self.pack()

    def _capture(self, batch, n, mb, nmb, nep):
        dev = self.device
        g = {"key": (tuple(int(batch[k].data_ptr()) for k in _BATCH_KEYS), n, mb, nmb, nep),
             "perm": torch.zeros((nep, n), dtype=torch.int64, device=dev), "mom": torch.zeros((nep, nmb, 2), device=dev),
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
        """`perms`: the epochs' permutations of the n rows (int64 tensors on the device).  Returns the mean statistics."""
        batch = self._prepare(batch)
        n, nep = int(batch["obs"].shape[0]), len(perms)
        self.set_hparams(lr, cliprange, ent_coef, vf_coef, max_grad_norm)
        self.stats.zero_()
        if self._graph_ok and world == 1:
            key = (tuple(int(batch[k].data_ptr()) for k in _BATCH_KEYS), n, mb, nmb, nep)
            if self._graph is None or self._graph["key"] != key:
                self._graph = None
                self._graph = self._capture(batch, n, mb, nmb, nep)
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
