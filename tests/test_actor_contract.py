"""The rollout head (fwgym_actor.h: fwg_actor_observe / fwg_actor_act = k_actor_stats + k_actor_act<SPLIT, NK1>) against float64 over
its whole shape contract -- obs_dim 1..64 (every NK1 = ceil(obs_dim / 16), both sides of every k-block boundary, the float4 and the
scalar load path), act_dim 1..4, batches with a tile edge (31 / 32 / 33 envs per wave tile, 255 / 256 / 257 per workgroup, one env),
VecNormalize's arguments, training and frozen statistics, the Philox noise stream -- so that a rewrite of the kernels for speed has
to keep what they compute:

  * the forward pass per element: the normalised observation against float64 statistics, mean and value against the float64
    networks on the kernel's own normalised observation (the matrix-core arithmetic alone) and end to end from the raw observation;
    every input buffer followed by 64 rows of NaN, every output buffer by 64 rows of a sentinel that must survive;
  * the single-product mode at NK1 = 2 and 3;
  * the running statistics: one env, two observe calls before one act, frozen -> training, discounted returns with gamma 0.9,
    set_stats -> get_stats, a first batch 10 and 100 standard deviations away from 0;
  * non-default gamma / clip_obs / clip_reward / epsilon with a third of the entries at the clip;
  * the sampling noise equal to the oracle's Philox stream 6 at (seed, env_id_base + env, number of acts before this one);
  * a captured pair of acts replayed three times equal to the eager sequence bit for bit (GPU).

The yardsticks are float64 numpy, written out below: the two 64-64 tanh networks, stable-baselines' RunningMeanStd / VecNormalize,
oracle.physics.rng_bits(seed, ids, counter, 6) -> box_muller.  The emulated forms (host build of the kernels, CPU) run the smallest
shapes that reach each path; tools/mutation_check.py re-runs them against kernel sources with a head bug put back
(FWGYM_MUTANT_SRC / FWGYM_MUTANT_TAG).  The error of an output x against its reference is |x - ref| / max(|ref|, 1), per element."""
import math
import os

import numpy as np
import pytest
import torch

from gym_fixed_wing import _native as nat
from gym_fixed_wing.actor import DeviceActor, weights_from_module
from gym_fixed_wing.rollout import MlpPolicy
from oracle import physics as oph

MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")
PAD = 64                      # guard rows behind every buffer
SENT, SENT_U8 = -777.25, 0xAB   # what the guard rows of the outputs hold
STREAM_POLICY = 6             # (FWG_STREAM_POLICY)
F32 = np.float32

# ---- bounds ----------------------------------------------------------------------------------------------------------------------
# mean and value, split-bf16 products: 2 x the worst error measured over the cases below (profiles/actor_contract_errors.txt); the
# margin is for other data seeds and box-to-box accumulation order.  May not pass 1e-4: one of the three products lost costs ~2^-9 of
# a term (>= 1e-3 here).  Host emulation: worst 3.66e-5 (n 257, D 32, A 4) on the kernel's own normalised observation; end to end
# 4.91e-5 for the one-row batch n 1, D 64, A 4 (its normalised observation carries the one-row conditioning of _obs_tol through the
# networks) and 3.66e-5 otherwise.  MI355X (the table is in the same file): 3.42e-5 and, for that one-row batch, 5.08e-5 end to end
# (7.7e-6 on the kernel's own normalised observation) -- both within these bounds, which stay.  A figure above a bound raises it to
# twice that figure, or, past 1e-4, is a finding about the kernel.
FWD_TOL_ISO = 7.4e-5   # against the float64 networks on the kernel's own normalised observation
FWD_TOL_E2E = 9.9e-5   # against float64 from the raw observation (adds the normalised observation's error through the networks)
assert FWD_TOL_ISO <= 1e-4 and FWD_TOL_E2E <= 1e-4
OBS_TOL = 5e-5       # normalised observation / reward, absolute (values up to clip = 10): tests/test_actor.py's bound
PLAIN_TOL = 6e-2     # single bf16 products, relative to the largest output of the batch (test_actor_plain_bf16_mode_is_close)
LOG_2PI_HALF = 0.5 * math.log(2 * math.pi)


def _obs_tol(ref, obs):
    """The bound on the normalised observation `obs` under the statistics of `ref`, per element: OBS_TOL, and for ONE-row batches
    what their conditioning adds.  There x - mean is a cancellation (after the first row mean = x / 1.0001 and var = 1e-4 (1 + x^2):
    1 / std up to 100) and the batch sums reach the fold as fixed-point integers of quantum 2^-20 (fwgym_env.h, FWG_ACC_SCALE):
      * the mean is off by half a quantum and by its own fp32 rounding: (2^-21 + 2^-23 |x|) / std;
      * the variance is off by _var_atol_one_row, which moves 1 / std: |normalised x| / (2 var) of it.
    From 31 rows on both terms are below 1e-7 and OBS_TOL stands alone."""
    if ref.ret.shape[0] > 1:
        return OBS_TOL
    rstd, x = ref.rstd(), np.abs(np.asarray(obs, np.float64))
    return OBS_TOL + rstd * (2.0 ** -21 + 2.0 ** -23 * x) + 0.5 * np.abs(ref.norm_obs(obs)) * rstd ** 2 * _var_atol_one_row(ref.dmax_obs)


def _var_rtol(ratio):
    """fp32 cancellation of s2 - s1^2 around the running mean the deviations are taken from (0 before the first fold): relative
    error of the variance <= 8 * 2^-24 * (1 + (mean / std)^2) -- 4.8e-5 at ratio 10, 4.8e-3 at ratio 100."""
    return 8 * 2.0 ** -24 * (1 + ratio ** 2)


def _var_atol_one_row(dmax):
    """One-row batches have std 0 and no ratio: there s1 and s2 are each off by half a fixed-point quantum (2^-21) and s1^2 by its
    fp32 rounding (2^-24 s1^2), so s2 - s1^2 is up to 2^-21 (1 + 2 |d|) + 2^-24 d^2 instead of 0, and the delta term s1^2 cnt n / tt
    carries s1's quantum too (<= 2^-20 |d|): together <= 2^-20 (1 + |d|)^2, d the batch's distance from the running mean."""
    return 2.0 ** -20 * (1 + dmax) ** 2


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def _emu():
    from emu.host_backend import HERE, HostBackend, build_emu
    path = build_emu(src=MUT_SRC, out=os.path.join(HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else build_emu()
    return nat.load_library(path), HostBackend()


def _gpu():
    from gym_fixed_wing.vec_env import _TorchBackend
    return nat.load_library(), _TorchBackend(0)


def _inp(mem, a, kind="f32"):
    """`a` on the device, followed by PAD rows of NaN (flags: 255)."""
    a = np.asarray(a)
    fill = np.full((PAD,) + a.shape[1:], np.nan, F32) if kind == "f32" else np.full((PAD,) + a.shape[1:], 255, np.uint8)
    return mem.from_host(np.concatenate([a.astype(fill.dtype), fill]), kind)


def _out(mem, n, cols=None, kind="f32"):
    return mem.full((n + PAD,) if cols is None else (n + PAD, cols), SENT if kind == "f32" else SENT_U8, kind)


def _weights(D, A, seed):
    """MlpPolicy's weights x 2.5 (tanh leaves its linear range) and nonzero biases -> dict of float32 arrays (torch layout)."""
    torch.manual_seed(seed)
    pol = MlpPolicy(D, act_dim=A)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([-0.3, 0.1, 0.4, -0.6][:A]))
        for p in pol.parameters():
            if p.dim() == 2:
                p.mul_(2.5)
            elif p is not pol.log_std:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return weights_from_module(pol)


class _Head(object):
    """A DeviceActor whose every call goes through guarded buffers."""

    def __init__(self, lib, mem, n, D, A, w, **kw):
        self.mem, self.n, self.D, self.A = mem, n, D, A
        self.actor = DeviceActor(n, D, act_dim=A, _backend=mem, _lib=lib, **kw)
        self.actor.load_policy(w)

    def _inputs(self, obs, rew, done):
        n = self.n
        full = (_inp(self.mem, obs), None if rew is None else _inp(self.mem, rew), None if done is None else _inp(self.mem, done, "u8"))
        return full, tuple(None if t is None else t[:n] for t in full)

    def observe(self, obs, rew=None, done=None):
        full, view = self._inputs(obs, rew, done)
        self.actor.observe(*view)
        return full   # (kept alive by the caller until the next synchronising call)

    def step(self, obs, rew=None, done=None, deterministic=True, observe=True):
        """observe() + act() on guarded buffers -> the outputs' first n rows on the host.  The guard rows must keep the sentinel,
        the rows before them must all have been written with finite values."""
        m, n = self.mem, self.n
        full, view = self._inputs(obs, rew, done)
        if observe:
            self.actor.observe(*view)
        outs = {"norm_obs": _out(m, n, self.D), "action": _out(m, n, self.A), "value": _out(m, n), "logp": _out(m, n)}
        if rew is not None:
            outs["norm_reward"] = _out(m, n)
        if done is not None:
            outs["done_out"] = _out(m, n, kind="u8")
        self.actor.act(view[0], reward=view[1], done=view[2], deterministic=deterministic, **{k: t[:n] for k, t in outs.items()})
        m.sync()
        res = {}
        for k, t in outs.items():
            h = np.array(m.to_host(t))
            sent = SENT_U8 if k == "done_out" else F32(SENT)
            assert np.all(h[n:] == sent), "{}: rows past n_envs written".format(k)
            if k != "done_out":
                assert np.all(np.isfinite(h[:n])) and not np.any(h[:n] == sent), "{}: a row left unwritten or not finite".format(k)
            res[k] = h[:n].copy()
        return res

    def stats(self):
        st = self.actor.get_stats()
        for k, v in st.items():
            assert np.all(np.isfinite(np.asarray(v))), (k, v)
        return st

    def close(self):
        self.actor.close()


# ---- the float64 yardsticks ------------------------------------------------------------------------------------------------------
def _mlp64(w, net, x):
    """One 64-64 tanh network of the weight dict `w` in float64: x [n][D] -> [n][out]."""
    g = lambda k: np.asarray(w["{}_{}".format(net, k)], np.float64)
    h = np.tanh(x @ g("w0").T + g("b0"))
    h = np.tanh(h @ g("w1").T + g("b1"))
    return h @ g("w2").T + g("b2")


class _Rms64(object):
    """stable-baselines' RunningMeanStd in float64."""

    def __init__(self, shape):
        self.mean, self.var, self.count = np.zeros(shape), np.ones(shape), 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        bm, bv, bc = x.mean(axis=0), x.var(axis=0), x.shape[0]
        delta, tot = bm - self.mean, self.count + bc
        m2 = self.var * self.count + bv * bc + delta ** 2 * self.count * bc / tot
        self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / tot, tot


class _VecNorm64(object):
    """stable-baselines' VecNormalize in float64 on the fp32 data: observe() = step_wait's bookkeeping for one batch, fold() = the
    moment the head's act publishes what it has seen.  Besides: the fp32 count sequence (count + batch rows, one fp32 add per
    fold), and for the variance bounds the largest |batch mean - running mean at the last fold| / batch std (ratio_*) and the
    largest such distance alone (dmax_*, per feature)."""

    def __init__(self, n, D, gamma=0.99, clip_obs=10.0, clip_rew=10.0, eps=1e-8, training=True):
        self.obs_rms, self.ret_rms, self.ret = _Rms64((D,)), _Rms64(()), np.zeros(n)
        self.gamma, self.clip_obs, self.clip_rew, self.eps = (float(F32(x)) for x in (gamma, clip_obs, clip_rew, eps))
        self.training = training
        self.count32, self.ret_count32 = F32(1e-4), F32(1e-4)
        self._pend, self._pend_ret = 0, 0
        self._base, self._base_ret = np.zeros(D), 0.0
        self.ratio_obs = self.ratio_ret = self.dmax_obs = self.dmax_ret = 0.0

    def set_stats(self, mean, var, count, ret_mean=0.0, ret_var=1.0, ret_count=1e-4):
        f = lambda x: np.asarray(x, F32).astype(np.float64)
        self.obs_rms.mean, self.obs_rms.var, self.obs_rms.count = f(mean), f(var), float(F32(count))
        self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count = float(F32(ret_mean)), float(F32(ret_var)), float(F32(ret_count))
        self.count32, self.ret_count32 = F32(count), F32(ret_count)
        self._base, self._base_ret = self.obs_rms.mean.copy(), self.ret_rms.mean

    @staticmethod
    def _track(x, base):
        x = np.asarray(x, np.float64)
        d, s = np.abs(x.mean(axis=0) - base), x.std(axis=0)
        return (float(np.max(d / s)) if x.shape[0] > 1 else 0.0), d

    def observe(self, obs, rew=None, done=None):
        if self.training:
            r, d = self._track(obs, self._base)
            self.ratio_obs, self.dmax_obs = max(self.ratio_obs, r), np.maximum(self.dmax_obs, d)
            self.obs_rms.update(obs)
            self._pend += obs.shape[0]
        if rew is not None:
            self.ret = self.ret * self.gamma + np.asarray(rew, np.float64)
            if self.training:
                r, d = self._track(self.ret, self._base_ret)
                self.ratio_ret, self.dmax_ret = max(self.ratio_ret, r), max(self.dmax_ret, float(d))
                self.ret_rms.update(self.ret)
                self._pend_ret += self.ret.shape[0]
            if done is not None:
                self.ret[np.asarray(done) != 0] = 0.0

    def fold(self):
        self.count32, self.ret_count32 = F32(self.count32 + F32(self._pend)), F32(self.ret_count32 + F32(self._pend_ret))
        self._pend = self._pend_ret = 0
        self._base, self._base_ret = self.obs_rms.mean.copy(), float(self.ret_rms.mean)

    def rstd(self):
        return 1.0 / np.sqrt(self.obs_rms.var + self.eps)

    def raw_obs(self, obs):
        return (np.asarray(obs, np.float64) - self.obs_rms.mean) * self.rstd()

    def raw_rew(self, rew):
        return np.asarray(rew, np.float64) / math.sqrt(self.ret_rms.var + self.eps)

    def norm_obs(self, obs):
        return np.clip(self.raw_obs(obs), -self.clip_obs, self.clip_obs)

    def norm_rew(self, rew):
        return np.clip(self.raw_rew(rew), -self.clip_rew, self.clip_rew)


def _err(x, ref):
    """The largest |x - ref| / max(|ref|, 1) over the elements."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return float(np.max(np.abs(x - ref) / np.maximum(np.abs(ref), 1.0)))


def _check_stats(head, ref, what="stats"):
    """The head's statistics against `ref`: mean rtol = atol = 2e-5, count exact (the fp32 sum), variance within _var_rtol of the
    worst-conditioned fold (one-row batches: + _var_atol_one_row).  -> (largest relative variance error, obs and returns)"""
    st = head.stats()
    one = head.n == 1
    np.testing.assert_allclose(st["obs_mean"], ref.obs_rms.mean, rtol=2e-5, atol=2e-5, err_msg=what)
    np.testing.assert_allclose(st["ret_mean"], ref.ret_rms.mean, rtol=2e-5, atol=2e-5, err_msg=what)
    assert F32(st["obs_count"]) == ref.count32 and F32(st["ret_count"]) == ref.ret_count32, (what, st["obs_count"], ref.count32, st["ret_count"], ref.ret_count32)
    assert abs(st["obs_count"] - ref.obs_rms.count) <= 1e-6 * ref.obs_rms.count, (what, st["obs_count"], ref.obs_rms.count)
    errs = []
    for got, want, ratio, dmax, key in ((st["obs_var"], ref.obs_rms.var, ref.ratio_obs, ref.dmax_obs, "obs_var"),
                                        (st["ret_var"], ref.ret_rms.var, ref.ratio_ret, ref.dmax_ret, "ret_var")):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        tol = _var_rtol(0.0) * want + _var_atol_one_row(dmax) if one else _var_rtol(ratio) * want
        assert np.all(np.abs(got - want) <= tol), (what, key, float(np.max(np.abs(got - want) / want)), ratio, np.max(dmax))
        errs.append(float(np.max(np.abs(got - want) / want)))
    return tuple(errs)


# ---- a. the forward pass over the shape contract ---------------------------------------------------------------------------------
def _run_forward(lib, mem, n, D, A, precise=True, steps=3):
    """Three observe / act steps (training statistics, deterministic; rewards and dones from the second on).  -> the worst errors
    and the last step's (mean, value) with their two float64 references."""
    seed = 1000 * D + 10 * A + n
    w = _weights(D, A, seed)
    rng = np.random.default_rng(seed)
    head = _Head(lib, mem, n, D, A, w, precise=precise, seed=11, env_id_base=5)
    ref = _VecNorm64(n, D)
    scale, shift = rng.uniform(0.5, 4.0, D).astype(F32), rng.uniform(-5, 5, D).astype(F32)
    worst = {k: 0.0 for k in ("obs", "obs_of_tol", "rew", "mean_iso", "value_iso", "mean_e2e", "value_e2e")}
    logp_det = float(-(np.asarray(w["log_std"], np.float64) + LOG_2PI_HALF).sum())
    last = None
    for t in range(steps):
        obs = (rng.normal(size=(n, D)).astype(F32) * scale + shift)
        rew = done = None
        if t > 0:
            rew = (rng.normal(size=n) * 3 - 1).astype(F32)
            done = (rng.uniform(size=n) < 0.2).astype(np.uint8)
        out = head.step(obs, rew, done, deterministic=True)
        ref.observe(obs, rew, done)
        ref.fold()
        w_no = ref.norm_obs(obs)
        e_obs = np.abs(out["norm_obs"] - w_no)
        worst["obs"] = max(worst["obs"], float(e_obs.max()))
        worst["obs_of_tol"] = max(worst["obs_of_tol"], float(np.max(e_obs / _obs_tol(ref, obs))))
        mine = out["norm_obs"].astype(np.float64)
        iso = (_mlp64(w, "pi", mine), _mlp64(w, "vf", mine)[:, 0])
        e2e = (_mlp64(w, "pi", w_no), _mlp64(w, "vf", w_no)[:, 0])
        for key, got, a, b in (("mean", out["action"], iso[0], e2e[0]), ("value", out["value"], iso[1], e2e[1])):
            worst[key + "_iso"] = max(worst[key + "_iso"], _err(got, a))
            worst[key + "_e2e"] = max(worst[key + "_e2e"], _err(got, b))
        np.testing.assert_allclose(out["logp"], np.full(n, logp_det), rtol=1e-5)
        if rew is not None:
            worst["rew"] = max(worst["rew"], float(np.abs(out["norm_reward"] - ref.norm_rew(rew)).max()))
            np.testing.assert_array_equal(out["done_out"], done)
        last = (out["action"], out["value"], iso, e2e)
    worst["obs_var"], worst["ret_var"] = _check_stats(head, ref, "forward")
    head.close()
    return worst, last


def _check_forward_case(lib, mem, where, n, D, A):
    worst, _ = _run_forward(lib, mem, n, D, A)
    print("ACTOR_CONTRACT forward {} n={} D={} A={}: ".format(where, n, D, A) + " ".join("{}={:.3g}".format(k, v) for k, v in worst.items()))
    assert worst["obs_of_tol"] <= 1.0 and worst["rew"] <= OBS_TOL, worst   # (obs_of_tol: the largest error / _obs_tol)
    assert worst["mean_iso"] <= FWD_TOL_ISO and worst["value_iso"] <= FWD_TOL_ISO, worst
    assert worst["mean_e2e"] <= FWD_TOL_E2E and worst["value_e2e"] <= FWD_TOL_E2E, worst


# (n, D, A), pairwise: between them D in {1, 3, 14, 16, 17, 32, 33, 48, 49, 60, 64} (both sides of every k-block boundary, every
# NK1, D % 4 == 0 -> float4 loads and the scalar path), A in 1..4, n in {1, 31, 32, 33, 255, 256, 257, 513} (one env, a wave tile and
# a workgroup -1 / 0 / +1, two workgroups and a tail)
GPU_FWD_CASES = [(1, 1, 1), (33, 17, 2), (257, 32, 4), (31, 33, 1), (255, 48, 4), (256, 49, 2), (32, 64, 3), (257, 3, 4), (513, 16, 3),
                 (513, 60, 1), (33, 14, 2), (1, 64, 4)]
EMU_FWD_CASES = [(1, 1, 1), (33, 17, 2), (257, 32, 4), (31, 49, 3), (32, 14, 1), (65, 64, 4)]


def _ids(cases):
    return ["n{}-D{}-A{}".format(*c) for c in cases]


@pytest.mark.parametrize("n,D,A", EMU_FWD_CASES, ids=_ids(EMU_FWD_CASES))
def test_forward_over_the_shape_contract_emulated(n, D, A):
    lib, mem = _emu()
    _check_forward_case(lib, mem, "emu", n, D, A)


@pytest.mark.gpu
@pytest.mark.parametrize("n,D,A", GPU_FWD_CASES, ids=_ids(GPU_FWD_CASES))
def test_forward_over_the_shape_contract_on_gpu(n, D, A):
    lib, mem = _gpu()
    _check_forward_case(lib, mem, "gpu", n, D, A)


# ---- b. single products ----------------------------------------------------------------------------------------------------------
def _check_plain_mode(lib, mem, where, n, D, A):
    """precise=False at this shape: close to float64 in test_actor.py's measure (relative to the largest output of the batch), and
    really another arithmetic than the split path, which meets its own bound on the same data."""
    (_, (mean1, val1, iso1, _)), (ws, (mean3, val3, _, _)) = (_run_forward(lib, mem, n, D, A, precise=p) for p in (False, True))
    rel = lambda x, r: float(np.abs(x - r).max() / np.abs(r).max())
    e_mean, e_val, diff = rel(mean1, iso1[0]), rel(val1, iso1[1]), rel(mean1, mean3)
    print("ACTOR_CONTRACT plain {} n={} D={} A={}: mean={:.3g} value={:.3g} against_split={:.3g}".format(where, n, D, A, e_mean, e_val, diff))
    assert e_mean < PLAIN_TOL and e_val < PLAIN_TOL, (e_mean, e_val)
    assert diff > 1e-5, diff
    assert max(ws["mean_iso"], ws["value_iso"]) <= FWD_TOL_ISO, ws


PLAIN_CASES = [(65, 24, 3), (33, 40, 2)]   # NK1 = 2, NK1 = 3


@pytest.mark.parametrize("n,D,A", PLAIN_CASES, ids=_ids(PLAIN_CASES))
def test_single_product_mode_emulated(n, D, A):
    lib, mem = _emu()
    _check_plain_mode(lib, mem, "emu", n, D, A)


@pytest.mark.gpu
@pytest.mark.parametrize("n,D,A", PLAIN_CASES, ids=_ids(PLAIN_CASES))
def test_single_product_mode_on_gpu(n, D, A):
    lib, mem = _gpu()
    _check_plain_mode(lib, mem, "gpu", n, D, A)


# ---- c. the running statistics ---------------------------------------------------------------------------------------------------
def _batch(rng, n, D, scale=2.0, shift=1.0):
    return (rng.normal(size=(n, D)) * scale + shift).astype(F32)


def _rewards(rng, n, p_done=0.2):
    return (rng.normal(size=n) * 3 - 1).astype(F32), (rng.uniform(size=n) < p_done).astype(np.uint8)


def _stats_one_env(lib, mem):
    """n = 1: every batch has variance 0."""
    n, D = 1, 3
    rng = np.random.default_rng(31)
    head, ref = _Head(lib, mem, n, D, 2, _weights(D, 2, 31)), _VecNorm64(n, D)
    for t in range(3):
        obs = _batch(rng, n, D)
        rew, done = _rewards(rng, n) if t else (None, None)
        out = head.step(obs, rew, done)
        ref.observe(obs, rew, done)
        ref.fold()
        assert np.all(np.abs(out["norm_obs"] - ref.norm_obs(obs)) <= _obs_tol(ref, obs))
    errs = _check_stats(head, ref, "one env")
    head.close()
    return errs


def _stats_two_observes(lib, mem):
    """Two observe calls on different batches (the second with rewards) before one act: both are folded."""
    n, D = 70, 5
    rng = np.random.default_rng(32)
    head, ref = _Head(lib, mem, n, D, 3, _weights(D, 3, 32)), _VecNorm64(n, D)
    keep = []
    for t in range(2):
        b1, b2 = _batch(rng, n, D), _batch(rng, n, D, 1.0, -2.0)
        rew, done = _rewards(rng, n)
        keep.append(head.observe(b1))
        out = head.step(b2, rew, done)
        ref.observe(b1)
        ref.observe(b2, rew, done)
        ref.fold()
        assert ref.obs_rms.count == pytest.approx(1e-4 + 2 * n * (t + 1))
        assert np.abs(out["norm_obs"] - ref.norm_obs(b2)).max() <= OBS_TOL
        assert np.abs(out["norm_reward"] - ref.norm_rew(rew)).max() <= OBS_TOL
    errs = _check_stats(head, ref, "two observes")
    head.close()
    return errs


def _stats_frozen_then_training(lib, mem):
    """training=False: three observe / act steps leave the statistics bit-identical; what they saw is not folded after
    configure(training=True) either, only the step that follows (the discounted returns advance all along, as VecNormalize's do)."""
    n, D = 70, 6
    rng = np.random.default_rng(33)
    head, ref = _Head(lib, mem, n, D, 3, _weights(D, 3, 33), training=False), _VecNorm64(n, D, training=False)
    given = (rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D), 500.0, 0.3, 2.0, 400.0)
    head.actor.set_stats(*given)
    ref.set_stats(*given)
    before = head.stats()
    for t in range(3):
        obs = _batch(rng, n, D)
        rew, done = _rewards(rng, n)
        out = head.step(obs, rew, done)
        ref.observe(obs, rew, done)
        ref.fold()
        assert np.abs(out["norm_obs"] - ref.norm_obs(obs)).max() <= OBS_TOL
        after = head.stats()
        for k in before:
            np.testing.assert_array_equal(np.asarray(after[k]), np.asarray(before[k]), err_msg="frozen statistics moved: " + k)
    head.actor.set_training(True)
    ref.training = True
    obs = _batch(rng, n, D)
    rew, done = _rewards(rng, n)
    out = head.step(obs, rew, done)
    ref.observe(obs, rew, done)
    ref.fold()
    assert np.abs(out["norm_obs"] - ref.norm_obs(obs)).max() <= OBS_TOL
    assert np.abs(out["norm_reward"] - ref.norm_rew(rew)).max() <= OBS_TOL
    errs = _check_stats(head, ref, "frozen -> training")
    head.close()
    return errs


def _stats_returns(lib, mem):
    """gamma = 0.9, 30 % dones, 5 steps: the discounted returns' statistics and the normalised rewards."""
    n, D = 130, 4
    rng = np.random.default_rng(34)
    head, ref = _Head(lib, mem, n, D, 3, _weights(D, 3, 34), gamma=0.9), _VecNorm64(n, D, gamma=0.9)
    for t in range(5):
        obs = _batch(rng, n, D)
        rew, done = _rewards(rng, n, 0.3)
        out = head.step(obs, rew, done)
        ref.observe(obs, rew, done)
        ref.fold()
        assert np.abs(out["norm_reward"] - ref.norm_rew(rew)).max() <= OBS_TOL, t
        _check_stats(head, ref, "returns, step {}".format(t))
    errs = _check_stats(head, ref, "returns")
    head.close()
    return errs


def _stats_round_trip(lib, mem):
    """set_stats -> get_stats at D = 64: the fp32 values given."""
    D = 64
    rng = np.random.default_rng(35)
    head = _Head(lib, mem, 5, D, 1, _weights(D, 1, 35))
    mean, var = rng.normal(size=D) * 7, rng.uniform(1e-3, 50, D)
    head.actor.set_stats(mean, var, 12345.0, -0.7, 3.5, 777.0)
    st = head.stats()
    np.testing.assert_array_equal(st["obs_mean"], mean.astype(F32))
    np.testing.assert_array_equal(st["obs_var"], var.astype(F32))
    assert (st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"]) == (12345.0, float(F32(-0.7)), 3.5, 777.0)
    head.close()
    return (0.0, 0.0)


def _stats_conditioning(lib, mem):
    """A first batch of 256 rows with std 1 and |mean| / std = 10 and = 100: the variance within 8 * 2^-24 (1 + ratio^2) -- 4.8e-5
    and 4.8e-3.  (Plain samples: a standardised batch would make the sums of squares integers that fp32 holds exactly.)"""
    n, D = 256, 4
    worst = []
    for ratio in (10.0, 100.0):
        rng = np.random.default_rng(36)
        obs = (rng.normal(size=(n, D)) + ratio * np.array([1, -1, 1, -1])).astype(F32)
        head, ref = _Head(lib, mem, n, D, 3, _weights(D, 3, 36)), _VecNorm64(n, D)
        head.step(obs)
        ref.observe(obs)
        ref.fold()
        assert abs(ref.ratio_obs - ratio) < 0.2 * ratio
        ref.ratio_obs = ratio   # the bound as stated, at the nominal ratio
        worst.append(_check_stats(head, ref, "ratio {}".format(ratio))[0])
        head.close()
    return tuple(worst)


STATS_CHECKS = {"one_env": _stats_one_env, "two_observes": _stats_two_observes, "frozen_then_training": _stats_frozen_then_training,
                "returns": _stats_returns, "round_trip": _stats_round_trip, "conditioning": _stats_conditioning}


def _check_statistics(lib, mem, where, check):
    errs = STATS_CHECKS[check](lib, mem)
    print("ACTOR_CONTRACT stats {} {}: variance errors {:.3g} {:.3g}".format(where, check, *errs))


@pytest.mark.parametrize("check", sorted(STATS_CHECKS))
def test_statistics_emulated(check):
    lib, mem = _emu()
    _check_statistics(lib, mem, "emu", check)


@pytest.mark.gpu
@pytest.mark.parametrize("check", sorted(STATS_CHECKS))
def test_statistics_on_gpu(check):
    lib, mem = _gpu()
    _check_statistics(lib, mem, "gpu", check)


# ---- d. clipping and VecNormalize's arguments ------------------------------------------------------------------------------------
REW_SIGMAS = 2.0   # rewards at 2 sigma of ret_var: 2.5 puts 60 % of these 100 rewards at the clip, the edge of the band asked for


def _check_clipping(lib, mem):
    n, D, A = 100, 7, 3
    rng = np.random.default_rng(2)
    kw = dict(gamma=0.9, clip_obs=2.5, clip_reward=1.5, epsilon=1e-2)
    head = _Head(lib, mem, n, D, A, _weights(D, A, 41), training=False, **kw)
    ref = _VecNorm64(n, D, 0.9, 2.5, 1.5, 1e-2, training=False)
    given = (rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D), 1000.0, 0.2, 1.7, 900.0)
    head.actor.set_stats(*given)
    ref.set_stats(*given)
    obs = (ref.obs_rms.mean + 3.0 * np.sqrt(ref.obs_rms.var) * rng.normal(size=(n, D))).astype(F32)
    rew = (REW_SIGMAS * math.sqrt(ref.ret_rms.var) * rng.normal(size=n)).astype(F32)
    done = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    out = head.step(obs, rew, done)
    for key, got, raw, clip in (("obs", out["norm_obs"], ref.raw_obs(obs), 2.5), ("rew", out["norm_reward"], ref.raw_rew(rew), 1.5)):
        frac = float(np.mean(np.abs(raw) > clip))
        assert 0.2 <= frac <= 0.6, (key, frac)   # the reference itself reaches the clip
        want = np.clip(raw, -clip, clip)
        clipped = np.abs(raw) > clip + 1e-6      # (within 1e-6 of the clip fp32 and float64 may fall on either side)
        np.testing.assert_array_equal(got[clipped], want[clipped].astype(F32), err_msg=key + ": not exactly at the clip")
        assert np.abs(got - want).max() <= 1e-6, (key, float(np.abs(got - want).max()))
        assert np.abs(got).max() <= clip
    np.testing.assert_array_equal(out["done_out"], done)
    head.close()


def test_clipping_and_arguments_emulated():
    _check_clipping(*_emu())


@pytest.mark.gpu
def test_clipping_and_arguments_on_gpu():
    _check_clipping(*_gpu())


# ---- e. sampling -----------------------------------------------------------------------------------------------------------------
def _check_sampling(lib, mem):
    """Deterministic and sampled acts alternating: the noise of act number c (every act counts) is the oracle's Philox stream 6 at
    (seed, env_id_base + env, c); a head whose env ids start one later draws the first head's rows 1.. as its rows 0.."""
    n, D, A = 257, 9, 4
    seed, base = (7 << 32) | 3, 1000
    w = _weights(D, A, 51)
    rng = np.random.default_rng(51)
    mean, var = rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D)
    head = _Head(lib, mem, n, D, A, w, training=False, seed=seed, env_id_base=base)
    other = _Head(lib, mem, n - 1, D, A, w, training=False, seed=seed, env_id_base=base + 1)
    for h in (head, other):
        h.actor.set_stats(mean, var, 1000.0)
    ls = np.asarray(w["log_std"], np.float64)
    sigma = np.exp(ls)
    counter = 0
    for rnd in range(3):
        obs = _batch(rng, n, D, 1.0, 0.0)
        det, det_o = head.step(obs, deterministic=True, observe=False), other.step(obs[1:], deterministic=True, observe=False)
        counter += 1
        smp, smp_o = head.step(obs, deterministic=False, observe=False), other.step(obs[1:], deterministic=False, observe=False)
        mu = det["action"].astype(np.float64)
        np.testing.assert_array_equal(smp["value"], det["value"])
        z = (smp["action"].astype(np.float64) - mu) / sigma
        want = oph.box_muller(oph.rng_bits(seed, base + np.arange(n), counter, STREAM_POLICY))[:, :A]
        counter += 1
        tol = 1e-5 * np.maximum(1.0, np.abs(mu) / sigma)   # (the action carries the mean: its fp32 rounding, in units of sigma)
        assert np.all(np.abs(z - want) <= tol), (rnd, float(np.max(np.abs(z - want) / tol)))
        logp = (-0.5 * want ** 2 - ls - LOG_2PI_HALF).sum(axis=1)
        np.testing.assert_allclose(smp["logp"], logp, rtol=1e-5)
        np.testing.assert_allclose(det["logp"], np.full(n, -(ls + LOG_2PI_HALF).sum()), rtol=1e-5)
        np.testing.assert_array_equal(det_o["action"], det["action"][1:])
        np.testing.assert_array_equal(smp_o["action"], smp["action"][1:])
        np.testing.assert_array_equal(smp_o["logp"], smp["logp"][1:])
    head.close(), other.close()


def test_sampling_noise_is_the_oracle_stream_emulated():
    _check_sampling(*_emu())


@pytest.mark.gpu
def test_sampling_noise_is_the_oracle_stream_on_gpu():
    _check_sampling(*_gpu())


# ---- f. a captured pair of acts --------------------------------------------------------------------------------------------------
def _check_captured_pair(lib, mem, n, D, A, w, seed, replays=3):
    """observe + act (sampled), observe + act (deterministic) captured once -- an even number of acts, one chain on one stream --
    and replayed three times on fresh observations copied into the captured input buffers: every output and the statistics equal
    the eager sequence's bit for bit.  (`w`: the policy's weights; tests/test_actor_contract_cnn.py runs this with a CNN policy.)"""
    rng = np.random.default_rng(seed)
    data = [(_batch(rng, n, D),) + _rewards(rng, n) for _ in range(1 + 2 * replays)]
    kinds = ("f32", "f32", "u8")

    def outputs():
        return {"norm_obs": _out(mem, n, D), "action": _out(mem, n, A), "value": _out(mem, n), "logp": _out(mem, n),
                "norm_reward": _out(mem, n), "done_out": _out(mem, n, kind="u8")}

    def call(actor, ins, outs, deterministic):
        obs, rew, done = (t[:n] for t in ins)
        actor.observe(obs, rew, done)
        actor.act(obs, reward=rew, done=done, deterministic=deterministic, **{k: t[:n] for k, t in outs.items()})

    actors = [DeviceActor(n, D, act_dim=A, seed=9, env_id_base=3, _backend=mem, _lib=lib) for _ in range(2)]
    for a in actors:
        a.load_policy(w)
        warm = outputs()
        call(a, [_inp(mem, x, k) for x, k in zip(data[0], kinds)], warm, True)   # (a first step: statistics away from their start)
    mem.sync()
    eager, graphed = actors
    want = []
    for k in range(2 * replays):
        outs = outputs()
        call(eager, [_inp(mem, x, kd) for x, kd in zip(data[1 + k], kinds)], outs, k % 2 == 1)
        want.append(outs)
    mem.sync()
    ins = [[_inp(mem, x, kd) for x, kd in zip(data[1 + j], kinds)] for j in range(2)]
    outs = [outputs(), outputs()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for j in range(2):
            call(graphed, ins[j], outs[j], j == 1)
    for r in range(replays):
        for j in range(2):
            for t, x, kd in zip(ins[j], data[1 + 2 * r + j], kinds):
                t.copy_(_inp(mem, x, kd))
            for k, t in outs[j].items():
                t.fill_(SENT_U8 if k == "done_out" else SENT)
        graph.replay()
        mem.sync()
        for j in range(2):
            for k, t in outs[j].items():
                assert torch.equal(t, want[2 * r + j][k]), (r, j, k)
                assert not bool((t[:n] == (SENT_U8 if k == "done_out" else SENT)).all()), (r, j, k)
    se, sg = eager.get_stats(), graphed.get_stats()
    for k in se:
        np.testing.assert_array_equal(np.asarray(sg[k]), np.asarray(se[k]), err_msg=k)
    for a in actors:
        a.close()


@pytest.mark.gpu
def test_captured_pair_of_acts_equals_the_eager_sequence_on_gpu():
    lib, mem = _gpu()
    _check_captured_pair(lib, mem, 257, 33, 2, _weights(33, 2, 61), 61)
