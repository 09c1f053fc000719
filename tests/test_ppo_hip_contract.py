"""The HIP PPO update (fwgym_learner.h) against float64 over its whole shape contract, so that a rewrite of the kernels for speed
has to keep what they compute:

  * fwg_ppo_grad (k_ppo_grad + k_ppo_reduce): the gradient and the loss sums of one minibatch for observation sizes 1..64, 1..4
    actions and minibatches of 1 to 65 536 rows -- tail tiles, more than 256 tiles split unevenly over the 256 workgroups --
    gathered through a permutation at an offset, every row outside the minibatch NaN; stale slabs of a larger call; a batch
    of equal advantages and one of large magnitudes (the clip coefficient < 1 in the apply step);
  * fwg_ppo_moments: 1, 3 and 128 minibatches read through a permutation, and a cancellation case;
  * a whole update (2 epochs x 4 minibatches) checked at every step against float64 at the learner's own state, and
    fwg_ppo_step equal to its two halves bit for bit;
  * the captured update equal to the eager one while lr and cliprange change between updates, with one capture;
  * fwg_actor_pack (the head repacked on the device) equal to fwg_actor_set_weights' host packing.

The yardsticks are float64: autograd of ppo_loss on a float64 copy of the policy (computed on the fp32 data), numpy moments, clip +
Adam written out below.  The emulated forms (host build of the kernels, CPU) run the smallest shapes that reach each code path;
tools/mutation_check.py re-runs them against kernel sources with a learner bug put back (FWGYM_MUTANT_SRC / FWGYM_MUTANT_TAG)."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gym_fixed_wing import _native as nat
from gym_fixed_wing.actor import DeviceActor
from gym_fixed_wing.learner import STAT_KEYS, HipLearner
from test_ppo_hip import CLIP, ENT, MAXN, VF, _batch, _compare, _gpu, _learner, _policy, _ref_grad

MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")
LR, BETAS, EPS = 2.5e-4, (0.9, 0.999), 1e-5   # (_learner's hyper-parameters, HipLearner's Adam defaults)
GPU = torch.device("cuda", 0)
# the returns' mean offset from the values in the batches below: with returns that are only noise around the values, the value
# gradient of a large minibatch cancels to 1/sqrt(mb) of its terms, and 1e-4 of it at 65 536 rows would be below the split-bf16
# network's precision per row (1.9e-4 measured on the MI355X for vf.4.bias: a bound on the data, not on the kernel)
RET_SHIFT = 0.5


def _emu():
    from emu.host_backend import HERE, HostBackend, build_emu
    path = build_emu(src=MUT_SRC, out=os.path.join(HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else build_emu()
    return nat.load_library(path), HostBackend()


def _ptr(t, offset=0):
    return ctypes.c_void_p(int(t.data_ptr()) + offset)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _policy_nz(D, A, seed):
    """_policy with nonzero biases (sb_init_ zeroes them)."""
    pol = _policy(D, seed, A)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in list(pol.pi) + list(pol.vf):
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return pol


def _policy64(pol):
    """A float64 CPU copy of `pol` (a learner's policy: its parameters are views of the learner's flat buffer)."""
    return copy.deepcopy(pol).cpu().double()


def _scattered(b, mb, seed, k=1):
    """The mb rows of `b` as minibatch k of a permutation of a buffer of (k + 2) mb + 64 rows, every other row NaN: a read of any
    row but idx[0:mb] turns the gradient into NaN.  -> (buffers, permutation, offset k mb of the minibatch's indices)"""
    N = (k + 2) * mb + 64
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    buf = {}
    for key, v in b.items():
        x = torch.full((N,) + tuple(v.shape[1:]), float("nan"), dtype=torch.float32)
        x[perm[k * mb:(k + 1) * mb]] = v
        buf[key] = x.contiguous()
    return buf, perm, k * mb


def _grad_and_stats(L, dbuf, dperm, off, mb):
    """fwg_ppo_moments + fwg_ppo_grad of the minibatch dperm[off:off + mb]; its statistics through fwg_ppo_apply on scratch copies
    of the state.  -> (gradient + loss sums, statistics)"""
    mom = torch.zeros(2, device=L.device)
    idx = dperm[off:off + mb]
    L.moments(dbuf, idx, mb, 1, mom)
    L.grad_half(L._batch_struct(dbuf), _ptr(idx), mb, _ptr(mom), L.grad)
    scratch = [t.clone() for t in (L.flat, L.exp_avg, L.exp_avg_sq, L.step, L.stats)]
    L.apply_half(L.grad, mb, *scratch)
    return L.grad.clone(), dict(zip(STAT_KEYS, scratch[4].cpu().tolist()))


def _check_stats(st, want, mb):
    """The loss sums within 1e-5 (pg_loss relative to the mean |term|), approx_kl within 3e-5, clip_frac exact as a count.
    (approx_kl = 0.5 mean (neglogp + old logp)^2 cancels two terms of ~6 to ~0.2 per row, so it carries the split-bf16 network's
    error of the mean action: 1.1e-5 at D = 64, A = 4 over 63 rows, 1e-7 over 4 097.)"""
    for k in ("pg_loss", "vf_loss", "entropy", "approx_kl"):
        scale = want["pg_scale"] if k == "pg_loss" else abs(want[k])
        tol = 3e-5 if k == "approx_kl" else 1e-5
        assert abs(st[k] - want[k]) <= tol * scale, (k, st[k], want[k])
    assert round(st["clip_frac"] * mb) == round(want["clip_frac"] * mb), (st["clip_frac"] * mb, want["clip_frac"] * mb)


def _clip_adam64(p, g, m, v, t, lr):
    """clip_grad_norm_(MAXN) + torch.optim.Adam(eps=1e-5) in float64 from the state (p, m, v, t), fed the gradient g.
    -> (parameters, m, v, clip coefficient)"""
    p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
    coef = min(MAXN / (float(g.norm()) + 1e-6), 1.0)
    g = g * coef
    b1, b2 = BETAS
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    t = t + 1
    p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + EPS)
    return p, m, v, coef


def _check_state(L, p, m, v):
    """_check_apply's bounds: parameters rtol 1e-6, both moments rtol 1e-6 (floor at 1e-6 of the moment vector's scale)."""
    np.testing.assert_allclose(_np(L.flat).astype(np.float64), p.numpy(), rtol=1e-6, atol=1e-7, err_msg="params")
    for mine, want, key in ((L.exp_avg, m, "exp_avg"), (L.exp_avg_sq, v, "exp_avg_sq")):
        np.testing.assert_allclose(_np(mine).astype(np.float64), want.numpy(), rtol=1e-6, atol=1e-6 * float(want.abs().max()), err_msg=key)


# ---- fwg_ppo_grad over the shape contract ------------------------------------------------------------------------------------
def _check_grad_case(lib, mem, device, D, A, mb, seed):
    pol = _policy_nz(D, A, seed)
    b = _batch(pol, mb, D, seed + 1, RET_SHIFT)
    want, st_want = _ref_grad(pol, b)
    buf, perm, off = _scattered(b, mb, seed + 2)
    pol = pol.to(device)
    L, actor = _learner(lib, mem, pol, device)
    grad, st = _grad_and_stats(L, {k: v.to(device) for k, v in buf.items()}, perm.to(device), off, mb)
    _compare(grad, pol, want)
    _check_stats(st, st_want, mb)
    actor.close()


# (D, A, mb): a tail tile (mb % 64 != 0) and more than 256 tiles (mb > 16 384: an uneven split over the 256 workgroups) each meet
# D = 1, D = 64, A = 1 and A = 4; 16 384 rows are exactly 256 tiles
GPU_GRAD_CASES = [(1, 1, 65), (1, 4, 3 * 16384 + 17), (64, 4, 63), (64, 1, 16385), (3, 2, 1), (12, 3, 64), (14, 2, 4097),
                  (33, 3, 16384), (60, 3, 65536), (12, 4, 65536), (60, 2, 16385)]
EMU_GRAD_CASES = [(1, 1, 65), (64, 4, 63), (3, 2, 1), (33, 3, 129), (14, 1, 16385)]


def _ids(cases):
    return ["D{}-A{}-mb{}".format(*c) for c in cases]


@pytest.mark.parametrize("D,A,mb", EMU_GRAD_CASES, ids=_ids(EMU_GRAD_CASES))
def test_gradient_over_the_shape_contract_emulated(D, A, mb):
    lib, mem = _emu()
    _check_grad_case(lib, mem, torch.device("cpu"), D, A, mb, 100 + D + 7 * A)


@pytest.mark.gpu
@pytest.mark.parametrize("D,A,mb", GPU_GRAD_CASES, ids=_ids(GPU_GRAD_CASES))
def test_gradient_over_the_shape_contract_on_gpu(D, A, mb):
    lib, mem = _gpu()
    _check_grad_case(lib, mem, GPU, D, A, mb, 100 + D + 7 * A)


def _check_no_stale_slabs(lib, mem, device, big, small):
    """A large minibatch, then a small one on the same learner: the second gradient sums only its own slabs."""
    pol = _policy_nz(12, 3, 21)
    cases = [(mb, _batch(pol, mb, 12, 22 + mb, RET_SHIFT)) for mb in (big, small)]
    wants = [_ref_grad(pol, b) for _, b in cases]
    pol = pol.to(device)
    L, actor = _learner(lib, mem, pol, device)
    for (mb, b), (want, st_want) in zip(cases, wants):
        buf, perm, off = _scattered(b, mb, 23 + mb)
        grad, st = _grad_and_stats(L, {k: v.to(device) for k, v in buf.items()}, perm.to(device), off, mb)
        _compare(grad, pol, want)
        _check_stats(st, st_want, mb)
    actor.close()


def test_small_minibatch_after_a_large_one_emulated():
    lib, mem = _emu()
    _check_no_stale_slabs(lib, mem, torch.device("cpu"), 300, 65)


@pytest.mark.gpu
def test_small_minibatch_after_a_large_one_on_gpu():
    lib, mem = _gpu()
    _check_no_stale_slabs(lib, mem, GPU, 65536, 65)


def _check_edge_batches(lib, mem, device, mb):
    # equal advantages: the normalised advantage is 0, the policy's gradient vanishes, log_std's is -ent_coef
    pol = _policy_nz(12, 3, 31)
    b = _batch(pol, mb, 12, 32, RET_SHIFT)
    b["adv"] = torch.full_like(b["adv"], 0.7)
    want, st_want = _ref_grad(pol, b)
    buf, perm, off = _scattered(b, mb, 33)
    pol = pol.to(device)
    L, actor = _learner(lib, mem, pol, device)
    grad, st = _grad_and_stats(L, {k: v.to(device) for k, v in buf.items()}, perm.to(device), off, mb)
    _compare(grad, pol, want)
    _check_stats(st, st_want, mb)
    g = grad[:L.num_params].cpu()
    A = pol.log_std.numel()
    assert torch.equal(g[:A], torch.full((A,), -ENT)), g[:A]
    o = A
    for name, p in list(pol.named_parameters())[1:]:
        if name.startswith("pi."):
            assert float(g[o:o + p.numel()].abs().max()) == 0.0, name
        o += p.numel()
    actor.close()
    # large magnitudes: advantages ~1e3, values ~1e2 and returns 20 above them: the gradient norm is far above max_grad_norm, so
    # the apply step clips
    pol = _policy_nz(12, 3, 34)
    with torch.no_grad():
        pol.vf[-1].bias.fill_(100.0)
    b = _batch(pol, mb, 12, 35, ret_shift=20.0)
    b["adv"] = (1e3 + 150.0 * b["adv"].double()).float()
    want, st_want = _ref_grad(pol, b)
    buf, perm, off = _scattered(b, mb, 36)
    pol = pol.to(device)
    L, actor = _learner(lib, mem, pol, device)
    dbuf = {k: v.to(device) for k, v in buf.items()}
    grad, st = _grad_and_stats(L, dbuf, perm.to(device), off, mb)
    _compare(grad, pol, want)
    _check_stats(st, st_want, mb)
    P = L.num_params
    p, m, v, coef = _clip_adam64(L.flat, grad[:P], L.exp_avg, L.exp_avg_sq, int(L.step.item()), LR)
    assert coef < 0.5, coef
    L.apply_half(grad, mb)
    _check_state(L, p, m, v)
    assert int(L.step.item()) == 1
    actor.close()


def test_edge_batches_emulated():
    lib, mem = _emu()
    _check_edge_batches(lib, mem, torch.device("cpu"), 65)


@pytest.mark.gpu
def test_edge_batches_on_gpu():
    lib, mem = _gpu()
    _check_edge_batches(lib, mem, GPU, 4097)


# ---- fwg_ppo_moments ---------------------------------------------------------------------------------------------------------
def _check_moments(lib, mem, device, nmb, mb, loc, scale, seed):
    """mean and biased std + 1e-8 of the advantages of nmb minibatches of a permutation (the entries past them point at NaN)."""
    L, actor = _learner(lib, mem, _policy(3, 0, 1).to(device), device)
    N = nmb * mb + 97
    g = torch.Generator().manual_seed(seed)
    adv = (loc + scale * torch.randn(N, generator=g, dtype=torch.float64)).float()
    perm = torch.randperm(N, generator=g)
    adv[perm[nmb * mb:]] = float("nan")
    out = torch.zeros(nmb, 2, device=device)
    L.moments({"adv": adv.to(device)}, perm.to(device), mb, nmb, out)
    a64 = adv.double()[perm[:nmb * mb]].view(nmb, mb).numpy()
    m64, s64 = a64.mean(axis=1), a64.std(axis=1)
    got = _np(out).astype(np.float64)
    err_m = np.abs(got[:, 0] - m64) / (1e-6 * s64 + 1e-7 * np.abs(m64))
    err_s = np.abs(got[:, 1] - (s64 + 1e-8)) / (1e-6 * (s64 + 1e-8))
    assert err_m.max() <= 1.0 and err_s.max() <= 1.0, (float(err_m.max()), float(err_s.max()))
    actor.close()


# (n_minibatches, mb, mean, std): mb never a multiple of 256; the last: cancellation (mean 1e3, std 1e-2)
EMU_MOMENT_CASES = [(1, 300, 0.3, 2.0), (3, 300, -0.5, 1.0), (128, 77, 0.3, 2.0), (3, 300, 1e3, 1e-2)]
GPU_MOMENT_CASES = [(1, 100003, 0.3, 2.0), (3, 65537, -0.5, 1.0), (128, 4097, 0.3, 2.0), (3, 65537, 1e3, 1e-2)]


@pytest.mark.parametrize("nmb,mb,loc,scale", EMU_MOMENT_CASES)
def test_advantage_moments_emulated(nmb, mb, loc, scale):
    lib, mem = _emu()
    _check_moments(lib, mem, torch.device("cpu"), nmb, mb, loc, scale, nmb + mb)


@pytest.mark.gpu
@pytest.mark.parametrize("nmb,mb,loc,scale", GPU_MOMENT_CASES)
def test_advantage_moments_on_gpu(nmb, mb, loc, scale):
    lib, mem = _gpu()
    _check_moments(lib, mem, GPU, nmb, mb, loc, scale, nmb + mb)


# ---- a whole update, step by step --------------------------------------------------------------------------------------------
def _decisions(p64, d):
    """float64 ratio, value change, clipped value and log-prob of the rows `d` under `p64`."""
    with torch.no_grad():
        mean, v = p64.pi(d["obs"]), p64.vf(d["obs"]).squeeze(-1)
        ls = p64.log_std
        nl = 0.5 * (((d["actions"] - mean) / ls.exp()) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * ls.numel() + ls.sum()
    return nl, v


def _margin(p64, d):
    nl, v = _decisions(p64, d)
    ratio, dv = torch.exp(-d["logp"] - nl), v - d["values"]
    vc = d["values"] + dv.clamp(-CLIP, CLIP)
    tie = torch.where(dv.abs() > CLIP, ((v - d["returns"]) ** 2 - (vc - d["returns"]) ** 2).abs(), torch.full_like(v, 1.0))
    return float(torch.stack([(ratio - 1 + CLIP).abs(), (ratio - 1 - CLIP).abs(), (dv + CLIP).abs(), (dv - CLIP).abs(), tie]).min())


def _nudge(p64, hb, rows, eps=1e-4):
    """The update carries some rows next to a decision of the loss (ratio at 1 +- clip, value change at +- clip, a tie of the
    clipped value loss), where fp32 and float64 may branch apart.  Such rows of `hb` (host fp32, in place) are moved 2 eps clear of
    it through their old log-prob, old value and return -- never the advantage, whose moments stand for the epoch.  -> the keys
    changed"""
    d = {k: hb[k][rows].double() for k in ("obs", "actions", "values", "logp", "returns")}
    nl, v = _decisions(p64, d)
    logp, ov, ret = d["logp"].clone(), d["values"].clone(), d["returns"].clone()
    ratio = torch.exp(-logp - nl)
    for bnd in (1 - CLIP, 1 + CLIP):
        near = (ratio - bnd).abs() < eps
        logp = torch.where(near, -nl - torch.log(bnd + torch.where(ratio >= bnd, 2 * eps, -2 * eps)), logp)
    dv = v - ov
    for bnd in (-CLIP, CLIP):
        near = (dv - bnd).abs() < eps
        ov = torch.where(near, v - bnd - torch.where(dv >= bnd, 2 * eps, -2 * eps), ov)
    dv = v - ov
    vc = ov + dv.clamp(-CLIP, CLIP)
    u = (v - vc).abs().clamp_min(eps)   # (l1 - l2 = (v - vc)(v + vc - 2 R))
    near = (dv.abs() > CLIP) & (((v - ret) ** 2 - (vc - ret) ** 2).abs() < eps)
    s = torch.where(v + vc - 2 * ret >= 0, 1.0, -1.0).double()
    ret = torch.where(near, 0.5 * (v + vc) - s * 2 * eps / u, ret)
    changed = []
    for k, new in (("logp", logp), ("values", ov), ("returns", ret)):
        if not torch.equal(new, d[k]):
            hb[k][rows] = new.float()
            changed.append(k)
    assert _margin(p64, {k: hb[k][rows].double() for k in d}) >= eps
    return changed


def _check_update(lib, mem, device, D, A, mb, seed, nmb=4, nep=2):
    """2 epochs x nmb minibatches through fwg_ppo_moments + fwg_ppo_grad + fwg_ppo_apply, eagerly.  At every step: the moments
    against numpy, the gradient against float64 autograd at the learner's own parameters, the apply against float64 clip + Adam
    from the learner's own m, v, t fed its gradient; a twin learner's fwg_ppo_step equal to the two halves bit for bit."""
    n = nmb * mb
    pol = _policy_nz(D, A, seed)
    hb = _batch(pol, n, D, seed + 1, RET_SHIFT)
    pol = pol.to(device)
    L, actor = _learner(lib, mem, pol, device)
    T, twin = _learner(lib, mem, copy.deepcopy(pol), device)
    db = {k: v.to(device) for k, v in hb.items()}   # (CPU: the same tensors)
    bs = L._batch_struct(db)
    P = L.num_params
    g = torch.Generator().manual_seed(seed + 2)
    for e in range(nep):
        perm = torch.randperm(n, generator=g)
        dperm = perm.to(device)
        mom = torch.zeros(nmb, 2, device=device)
        L.moments(db, dperm, mb, nmb, mom)
        a64 = hb["adv"].double()[perm].view(nmb, mb)
        m64, s64 = a64.mean(1), a64.std(1, unbiased=False)
        got = _np(mom).astype(np.float64)
        assert np.all(np.abs(got[:, 0] - m64.numpy()) <= 1e-6 * s64.numpy() + 1e-7 * m64.abs().numpy()), (e, got, m64)
        assert np.all(np.abs(got[:, 1] - (s64.numpy() + 1e-8)) <= 1e-6 * (s64.numpy() + 1e-8)), (e, got, s64)
        for k in range(nmb):
            rows = perm[k * mb:(k + 1) * mb]
            p64 = _policy64(pol)
            for key in _nudge(p64, hb, rows):
                db[key].copy_(hb[key])
            want, _ = _ref_grad(p64, {key: v[rows] for key, v in hb.items()})
            idx, mk = _ptr(dperm, 8 * k * mb), _ptr(mom, 8 * k)
            L.grad_half(bs, idx, mb, mk, L.grad)
            _compare(L.grad, pol, want)
            p, m, v, _ = _clip_adam64(L.flat, L.grad[:P], L.exp_avg, L.exp_avg_sq, int(L.step.item()), LR)
            L.apply_half(L.grad, mb)
            _check_state(L, p, m, v)
            T.full_step(bs, idx, mb, mk)
            for name in ("flat", "exp_avg", "exp_avg_sq", "step", "stats"):
                assert torch.equal(getattr(L, name), getattr(T, name)), (e, k, name)
    assert int(L.step.item()) == nep * nmb
    actor.close(), twin.close()


def test_update_step_by_step_emulated():
    lib, mem = _emu()
    _check_update(lib, mem, torch.device("cpu"), 12, 3, 70, 41)


@pytest.mark.gpu
def test_update_step_by_step_on_gpu():
    lib, mem = _gpu()
    _check_update(lib, mem, GPU, 12, 3, 16385, 41)


# ---- the captured update equals the eager one --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_update_equals_the_eager_one_across_hparam_changes_on_gpu():
    lib, mem = _gpu()
    D, A, mb, nmb, nep = 12, 3, 4097, 4, 2
    n = mb * nmb
    pol = _policy_nz(D, A, 51)
    db = {k: v.to(GPU) for k, v in _batch(pol, n, D, 52, RET_SHIFT).items()}
    run = {}
    for graph in (True, False):
        actor = DeviceActor(256, D, act_dim=A, training=False, _backend=mem, _lib=lib)
        run[graph] = (HipLearner(lib, actor, copy.deepcopy(pol).to(GPU), GPU, graph=graph), actor)
    G, E = run[True][0], run[False][0]
    g = torch.Generator().manual_seed(53)
    first = None
    for lr, clip in ((2.5e-4, 0.2), (1e-4, 0.1), (6e-4, 0.3)):
        perms = [torch.randperm(n, generator=g).to(GPU) for _ in range(nep)]
        sg = G.update(db, perms, mb, nmb, lr, clip, ENT, VF, MAXN)
        se = E.update(db, perms, mb, nmb, lr, clip, ENT, VF, MAXN)
        if first is None:
            first = (G._graph, G._graph["graph"])
        assert G._graph is first[0] and G._graph["graph"] is first[1], "the update was captured again"
        assert E._graph is None
        assert sg == se, (lr, clip, sg, se)
        for name in ("flat", "exp_avg", "exp_avg_sq", "step", "stats"):
            assert torch.equal(getattr(G, name), getattr(E, name)), (lr, clip, name)
    assert int(G.step.item()) == 3 * nep * nmb
    # the heads repacked inside the graph and eagerly: the same actions and values
    obs = torch.randn(256, D, generator=torch.Generator().manual_seed(54)).to(GPU)
    outs = []
    for graph in (True, False):
        actor = run[graph][1]
        actor.set_stats(np.zeros(D), np.ones(D), 1000.0)
        outs.append([_np(x).copy() for x in actor.act(obs, deterministic=True)[1:4]])
        actor.close()
    for name, x, y in zip(("mean", "value", "logp"), *outs):
        np.testing.assert_array_equal(x, y, err_msg=name)


# ---- fwg_actor_pack equals the host packing ----------------------------------------------------------------------------------
def _check_pack(lib, mem, device, D, A, n):
    """One set of parameters loaded through fwg_actor_set_weights (load_policy) and through fwg_actor_pack: deterministic act()
    on the same observations and frozen statistics gives the same bits, and the head matches float64 torch."""
    pol = _policy_nz(D, A, 60 + 5 * D + A)
    rng = np.random.default_rng(D * 10 + A)
    mean, var = rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D)
    obs = mem.from_host((rng.normal(size=(n, D)) * 2).astype(np.float32))
    for precise in (True, False):
        host = DeviceActor(n, D, act_dim=A, training=False, precise=precise, _backend=mem, _lib=lib)
        host.load_policy(pol)
        dev = DeviceActor(n, D, act_dim=A, training=False, precise=precise, _backend=mem, _lib=lib)
        L = HipLearner(lib, dev, copy.deepcopy(pol).to(device), device, graph=False)
        L.pack()
        outs = []
        for a in (host, dev):
            a.set_stats(mean, var, 1000.0)
            outs.append([_np(x).copy() for x in a.act(obs, deterministic=True)[:4]])
        for name, x, y in zip(("norm_obs", "mean", "value", "logp"), *outs):
            np.testing.assert_array_equal(y, x, err_msg="{} (precise={})".format(name, precise))
        # test_actor.py's bounds, relative to the largest output of the batch: 2e-5 (split bf16), 6e-2 (plain bf16)
        p64 = copy.deepcopy(pol).double()
        with torch.no_grad():
            no = torch.from_numpy(outs[1][0]).double()
            w_mean, w_val = p64.pi(no).numpy(), p64.vf(no).squeeze(-1).numpy()
        tol = 2e-5 if precise else 6e-2
        for name, got, w in (("mean", outs[1][1], w_mean), ("value", outs[1][2], w_val)):
            err = float(np.abs(got - w).max() / np.abs(w).max())
            assert err < tol, (name, precise, err)
        host.close(), dev.close()


@pytest.mark.parametrize("D,A", [(1, 4), (64, 1), (14, 3)])
def test_device_repack_equals_host_packing_emulated(D, A):
    lib, mem = _emu()
    _check_pack(lib, mem, torch.device("cpu"), D, A, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 12, 14, 60, 64])
@pytest.mark.parametrize("A", [1, 3, 4])
def test_device_repack_equals_host_packing_on_gpu(D, A):
    lib, mem = _gpu()
    _check_pack(lib, mem, GPU, D, A, 4096)
