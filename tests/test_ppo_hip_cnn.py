"""PPO(update="hip_cnn"): the HIP PPO update of the CNN controller's CnnMlpPolicy (fwg_learner_create_cnn, k_ppo_grad<true>: the
backward pass through the conv shared by pi and vf) against float64, with test_ppo_hip_contract.py's yardsticks and bounds:

  * the gradient (all 15 tensors) and the loss sums over the shape contract -- observation size 60, 1..4 actions, one row, tail
    tiles, a workgroup that walks two tiles (the conv sums accumulate across tiles), an uneven split -- gathered through a
    permutation at an offset with every other row NaN; stale slabs of a larger call;
  * a whole update step by step against float64 at the learner's own state, fwg_ppo_step equal to its halves bit for bit;
  * the captured update equal to the eager one across lr / cliprange changes, with one capture;
  * fwg_actor_pack (conv included) equal to fwg_actor_set_weights + fwg_actor_set_conv from the host;
  * through PPO on the cnn configuration against the torch update; refusals, lifecycle and the build's resource report.

Each behaviour has an emulated form (host build of the kernels, CPU) and a `gpu` form; tools/mutation_check.py re-runs the emulated
forms against kernel sources with a bug put back (FWGYM_MUTANT_SRC, through test_ppo_hip_contract._emu).  The data-parallel path
(gradient half -> all-reduce -> apply half) is shared code over the flat gradient and is not tested again here
(tests/test_ppo_hip.py::test_two_rank_hip_learner_keeps_one_set_of_weights)."""
import copy
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import configs
from gym_fixed_wing import _native as nat
from gym_fixed_wing import specialize
from gym_fixed_wing.actor import DeviceActor
from gym_fixed_wing.learner import STAT_KEYS, HipLearner
from gym_fixed_wing.ppo import PPO, sb_init_
from gym_fixed_wing.rollout import CnnMlpPolicy, MlpPolicy
from test_ppo_hip import CLIP, ENT, MAXN, VF, _batch, _compare, _gpu, _ref_grad
from test_ppo_hip_contract import (LR, RET_SHIFT, _check_state, _check_stats, _clip_adam64, _emu, _grad_and_stats, _np, _nudge,
                                   _policy64, _ptr, _scattered)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GPU = torch.device("cuda", 0)
D = 60   # the 5 x 12 window
CPU = torch.device("cpu")


def _cnn_policy(A, seed):
    """test_ppo_hip._policy / test_ppo_hip_contract._policy_nz for the CnnMlpPolicy: stable-baselines' initialisation, nonzero
    biases (the conv's too), _policy's log-std, means of order 1."""
    torch.manual_seed(seed)
    pol = sb_init_(CnnMlpPolicy(act_dim=A))
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([-0.4, 0.3, -0.9, 0.1][:A]))
        pol.pi[-1].weight.mul_(40.0)
        pol.conv.bias.copy_(0.3 * torch.randn(pol.conv.bias.shape, generator=g))
        for m in list(pol.pi) + list(pol.vf):
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return pol


def _cnn_learner(lib, mem, pol, device, n=4, graph=False, **actor_kw):
    actor = DeviceActor(n, D, act_dim=pol.log_std.numel(), _backend=mem, _lib=lib, **actor_kw)
    actor.load_policy(pol)   # (makes it a CNN head: fwg_actor_set_conv)
    assert actor.cnn
    L = HipLearner(lib, actor, pol, device, graph=graph)
    L.set_hparams(LR, CLIP, ENT, VF, MAXN)
    return L, actor


def test_flat_layout_is_the_policy_s_parameter_order_emulated():
    lib, mem = _emu()
    for A in (1, 3, 4):
        pol = _cnn_policy(A, 1)
        names = [k for k, _ in pol.named_parameters()]
        assert names == ["log_std", "conv.weight", "conv.bias"] + ["{}.{}.{}".format(n, i, w) for n in ("pi", "vf") for i in (1, 3, 5)
                                                                   for w in ("weight", "bias")]
        assert tuple(pol.conv.weight.shape) == (5, 3) and tuple(pol.pi[1].weight.shape) == (64, 36)
        L, actor = _cnn_learner(lib, mem, pol, CPU)
        assert L.num_params == A + 18 + 2 * (64 * 36 + 64 + 64 * 64 + 64) + 65 * A + 65
        assert L.num_params == 13337 or A != 3
        actor.close()


# ---- the gradient over the shape contract ------------------------------------------------------------------------------------
def _check_grad_case(lib, mem, device, A, mb, seed):
    pol = _cnn_policy(A, seed)
    b = _batch(pol, mb, D, seed + 1, RET_SHIFT)
    want, st_want = _ref_grad(pol, b)
    names = [k for k, _ in pol.named_parameters()]
    norms = {k: float(w.norm()) for k, w in zip(names, want)}
    if mb == 1:   # (one row: its normalised advantage is 0 -- the gradient reaches the conv through vf alone)
        assert norms["pi.1.weight"] == 0.0 and norms["vf.1.weight"] > 1e-2, norms
        # ... and approx_kl = 0.5 kl^2 is ONE row's kl = neglogp + old logp, two terms of ~6 cancelling to <= 0.51: _check_stats'
        # 3e-5 of it allows kl an error of 1.5e-5 |kl|, and kl moves by sum_a |z_a| / sigma_a x the error of mean a.  The row is
        # chosen (float64, from the inputs alone: ONE_ROW_SEED) with |kl| >= 0.4 and that sensitivity x |mean| <= 1.5 |kl|, so
        # the bound sits >= 10x above the split-bf16 network's typical 1e-6 relative error of the mean
        p64 = _policy64(pol)
        with torch.no_grad():
            mu, sig = p64.pi(b["obs"].double())[0], p64.log_std.exp()
            sens = float((((b["actions"].double()[0] - mu) / sig).abs() * mu.abs() / sig).sum())
        kl = math.sqrt(2.0 * st_want["approx_kl"])
        assert kl >= 0.4 and sens <= 1.5 * kl, (kl, sens)
    assert norms["conv.weight"] > 1e-3 and norms["conv.bias"] > 1e-3, norms   # >= 10x _compare's floor of 1e-4: the bound is relative
    buf, perm, off = _scattered(b, mb, seed + 2)
    pol = pol.to(device)
    L, actor = _cnn_learner(lib, mem, pol, device)
    grad, st = _grad_and_stats(L, {k: v.to(device) for k, v in buf.items()}, perm.to(device), off, mb)
    assert len(want) == 15
    _compare(grad, pol, want)
    _check_stats(st, st_want, mb)
    actor.close()


# (A, mb).  1 row; 63 / 65 rows: tail tiles; 64: one full tile; 16 449 rows = 257 tiles, the smallest minibatch in which a
# workgroup (the last of the 256) walks two tiles; 49 169 rows: 769 tiles split unevenly over the 256 workgroups
EMU_GRAD_CASES = [(3, 1), (4, 63), (1, 65), (3, 129), (2, 16449)]
GPU_GRAD_CASES = [(3, 1), (4, 63), (1, 64), (3, 65), (3, 4097), (2, 16449), (3, 49169)]


def _ids(cases):
    return ["A{}-mb{}".format(*c) for c in cases]


ONE_ROW_SEED = 546   # (the first seed >= 500 whose single row meets _check_grad_case's conditions on the inputs)


def _seed(A, mb):
    return ONE_ROW_SEED if mb == 1 else 203 + 7 * A + (mb % 11)


@pytest.mark.parametrize("A,mb", EMU_GRAD_CASES, ids=_ids(EMU_GRAD_CASES))
def test_cnn_gradient_over_the_shape_contract_emulated(A, mb):
    lib, mem = _emu()
    _check_grad_case(lib, mem, CPU, A, mb, _seed(A, mb))


@pytest.mark.gpu
@pytest.mark.parametrize("A,mb", GPU_GRAD_CASES, ids=_ids(GPU_GRAD_CASES))
def test_cnn_gradient_over_the_shape_contract_on_gpu(A, mb):
    lib, mem = _gpu()
    _check_grad_case(lib, mem, GPU, A, mb, _seed(A, mb))


def _check_no_stale_slabs(lib, mem, device, big, small):
    """A large minibatch, then a small one on the same learner: the second gradient (the conv's entries too) sums only its own
    slabs."""
    pol = _cnn_policy(3, 21)
    cases = [(mb, _batch(pol, mb, D, 22 + mb, RET_SHIFT)) for mb in (big, small)]
    wants = [_ref_grad(pol, b) for _, b in cases]
    pol = pol.to(device)
    L, actor = _cnn_learner(lib, mem, pol, device)
    for (mb, b), (want, st_want) in zip(cases, wants):
        buf, perm, off = _scattered(b, mb, 23 + mb)
        grad, st = _grad_and_stats(L, {k: v.to(device) for k, v in buf.items()}, perm.to(device), off, mb)
        _compare(grad, pol, want)
        _check_stats(st, st_want, mb)
    actor.close()


def test_cnn_small_minibatch_after_a_large_one_emulated():
    lib, mem = _emu()
    _check_no_stale_slabs(lib, mem, CPU, 16449, 65)


@pytest.mark.gpu
def test_cnn_small_minibatch_after_a_large_one_on_gpu():
    lib, mem = _gpu()
    _check_no_stale_slabs(lib, mem, GPU, 16449, 65)


# ---- a whole update, step by step --------------------------------------------------------------------------------------------
def _check_update(lib, mem, device, A, mb, seed, nmb=4, nep=2):
    """test_ppo_hip_contract._check_update on the CnnMlpPolicy: 2 epochs x nmb minibatches through fwg_ppo_moments + fwg_ppo_grad
    + fwg_ppo_apply, eagerly.  At every step: the moments against numpy, the gradient against float64 autograd at the learner's
    own parameters, the apply against float64 clip + Adam from the learner's own m, v, t fed its gradient; a twin learner's
    fwg_ppo_step equal to the two halves bit for bit."""
    n = nmb * mb
    pol = _cnn_policy(A, seed)
    hb = _batch(pol, n, D, seed + 1, RET_SHIFT)
    pol = pol.to(device)
    L, actor = _cnn_learner(lib, mem, pol, device)
    T, twin = _cnn_learner(lib, mem, copy.deepcopy(pol), device)
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


def test_cnn_update_step_by_step_emulated():
    lib, mem = _emu()
    _check_update(lib, mem, CPU, 3, 70, 41)


@pytest.mark.gpu
def test_cnn_update_step_by_step_on_gpu():
    lib, mem = _gpu()
    _check_update(lib, mem, GPU, 3, 4097, 41)


# ---- the captured update equals the eager one --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cnn_captured_update_equals_the_eager_one_across_hparam_changes_on_gpu():
    lib, mem = _gpu()
    A, mb, nmb, nep = 3, 1025, 4, 2
    n = mb * nmb
    pol = _cnn_policy(A, 51)
    db = {k: v.to(GPU) for k, v in _batch(pol, n, D, 52, RET_SHIFT).items()}
    run = {}
    for graph in (True, False):
        L, actor = _cnn_learner(lib, mem, copy.deepcopy(pol).to(GPU), GPU, n=256, graph=graph, training=False)
        run[graph] = (L, actor)
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
    assert not torch.equal(G.policy.conv.weight.detach().cpu(), pol.conv.weight.detach())
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
def _check_pack(lib, mem, device, A, n):
    """One CnnMlpPolicy loaded through fwg_actor_set_weights + fwg_actor_set_conv (load_policy) and through fwg_actor_pack into a
    head that held ANOTHER policy's conv: deterministic act() on the same observations and frozen statistics gives the same
    bits, and the head matches float64 torch within test_actor.py's bounds."""
    pol, other = _cnn_policy(A, 60 + A), _cnn_policy(A, 90 + A)
    with torch.no_grad():   # (every conv entry differs: a pack that leaves any of them behind shows)
        assert float((pol.conv.weight - other.conv.weight).abs().min()) > 1e-3 and float((pol.conv.bias - other.conv.bias).abs().min()) > 1e-3
    rng = np.random.default_rng(600 + A)
    mean, var = rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D)
    obs = mem.from_host((rng.normal(size=(n, D)) * 2).astype(np.float32))
    for precise in (True, False):
        host = DeviceActor(n, D, act_dim=A, training=False, precise=precise, _backend=mem, _lib=lib)
        host.load_policy(pol)
        dev = DeviceActor(n, D, act_dim=A, training=False, precise=precise, _backend=mem, _lib=lib)
        dev.load_policy(other)
        L = HipLearner(lib, dev, copy.deepcopy(pol).to(device), device, graph=False)
        outs = []
        for a in (host, dev, dev):
            if len(outs) == 2:
                L.pack()
            a.set_stats(mean, var, 1000.0)
            outs.append([_np(x).copy() for x in a.act(obs, deterministic=True)[:4]])
        assert np.abs(outs[1][2] - outs[0][2]).max() > 1e-3   # (before the pack: the other policy)
        for name, x, y in zip(("norm_obs", "mean", "value", "logp"), outs[0], outs[2]):
            np.testing.assert_array_equal(y, x, err_msg="{} (precise={})".format(name, precise))
        # test_actor.py's bounds, relative to the largest output of the batch: 2e-5 (split bf16), 6e-2 (plain bf16)
        p64 = copy.deepcopy(pol).double()
        with torch.no_grad():
            no = torch.from_numpy(outs[2][0]).double()
            w_mean, w_val = p64.pi(no).numpy(), p64.vf(no).squeeze(-1).numpy()
        tol = 2e-5 if precise else 6e-2
        for name, got, w in (("mean", outs[2][1], w_mean), ("value", outs[2][2], w_val)):
            err = float(np.abs(got - w).max() / np.abs(w).max())
            assert err < tol, (name, precise, err)
        host.close(), dev.close()


@pytest.mark.parametrize("A", [1, 3, 4])
def test_cnn_device_repack_equals_host_packing_emulated(A):
    lib, mem = _emu()
    _check_pack(lib, mem, CPU, A, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 3, 4])
def test_cnn_device_repack_equals_host_packing_on_gpu(A):
    lib, mem = _gpu()
    _check_pack(lib, mem, GPU, A, 4096)


# ---- through PPO on the cnn configuration ------------------------------------------------------------------------------------
def _emu_vec(n=70, seed=3):
    """tests/test_cnn_policy.py's emulated env: the cnn configuration, a lagged 5 x 12 window on the row log."""
    from emu.host_backend import HostBackend
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    lib_path = _emu()[0]._name
    vec = FixedWingVecEnv(configs.reference_like("cnn"), num_envs=n, config_kw={"observation": {"step": 2}, "steps_max": 25}, seed=seed,
                          _backend=HostBackend(), _lib_path=lib_path, obs_log_rows=10)
    assert vec.obs_log_rows > 0 and tuple(vec.obs_shape) == (5, 12)
    vec.set_curriculum_level(0.25)
    vec.reset()
    return vec


def _composed(vec, update, batch=None, **kw):
    """PPO with `update` on `vec` and a CnnMlpPolicy of seed 0; one update of 2 epochs x 4 minibatches on `batch` (collected
    here when None)."""
    torch.manual_seed(0)
    net = sb_init_(CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3))
    ppo = PPO(vec, policy=net, seed=0, n_steps=16, nminibatches=4, noptepochs=2, update=update, **kw)
    w0 = torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()]).clone()
    if batch is None:
        batch = {k: v.clone() for k, v in ppo.collect().items()}
    stats = ppo.update({k: v.clone() for k, v in batch.items()})
    w1 = torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()]).clone()
    return ppo, batch, w0, w1, stats


def _check_composed(make_vec):
    """test_ppo_hip._check_composed's bounds, "torch" against "hip_cnn"."""
    vec = make_vec()
    pt, batch, w0, wt, st_t = _composed(vec, "torch")
    ph, _, w0h, wh, st_h = _composed(vec, "hip_cnn", batch)
    assert isinstance(ph.learner, HipLearner) and ph.learner.num_params == 13337 and ph.actor.cnn
    assert torch.equal(w0.cpu(), w0h.cpu())
    rel = float((wh - wt).norm() / (wt - w0).norm())
    print("hip_cnn against torch: |w_hip - w_torch| / |w_torch - w0| = {:.3e}".format(rel))
    assert rel <= 1e-2, rel
    for k in STAT_KEYS:
        assert st_h[k] == pytest.approx(st_t[k], rel=2e-2, abs=1e-4), (k, st_h[k], st_t[k])
    n_conv = 18
    A = ph.policy.log_std.numel()
    assert float((wh[A:A + n_conv] - w0[A:A + n_conv]).abs().min()) > 0.0   # the conv moved
    # determinism: the same update again from the same start, bit for bit
    ph2, _, _, wh2, _ = _composed(vec, "hip_cnn", batch)
    assert torch.equal(wh, wh2)
    return vec, ph, batch


def _check_head(vec, ppo):
    """The head (reading the row log's window in place) holds the learner's weights: its value against policy.vf on the head's
    own normalised observation."""
    no, _, value, _, _ = ppo.actor.act(vec._obs_buf, deterministic=True)
    with torch.no_grad():
        want = ppo.policy.vf(torch.as_tensor(_np(torch.as_tensor(no))).to(ppo._torch_dev)).squeeze(-1).cpu().numpy()
    np.testing.assert_allclose(_np(torch.as_tensor(value)), want, rtol=2e-3, atol=2e-3)
    assert np.abs(want).max() > 0


def test_hip_cnn_update_matches_the_torch_update_emulated(tmp_path):
    vec, ph, batch = _check_composed(_emu_vec)
    _check_head(vec, ph)   # (no host packing call since the update)
    # save -> load reproduces the weights (the module's parameters are views of the learner's buffer)
    ph.save(str(tmp_path / "m.npz"))
    w = [p.detach().clone() for p in ph.policy.parameters()]
    with torch.no_grad():
        for p in ph.policy.parameters():
            p.zero_()
    assert float(ph.learner.flat.abs().sum()) == 0.0
    ph.load(str(tmp_path / "m.npz"))
    for p, q in zip(ph.policy.parameters(), w):
        assert torch.equal(p.detach(), q)
    assert torch.equal(ph.learner.flat, torch.cat([q.reshape(-1) for q in w]))
    vec.close()


def test_training_loop_with_the_hip_cnn_update_emulated():
    from gym_fixed_wing.distributed import CurriculumSchedule
    vec = _emu_vec()
    torch.manual_seed(0)
    net = sb_init_(CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3))
    ppo = PPO(vec, policy=net, seed=0, n_steps=16, nminibatches=2, noptepochs=2, update="hip_cnn",
              curriculum=CurriculumSchedule(level=0.25, cooldown=1))
    before = copy.deepcopy(ppo.policy.state_dict())
    logs = []
    ppo.learn(2 * 16 * 70, log=logs.append)
    assert ppo.updates == 2 and ppo.num_timesteps == 2 * 16 * 70
    assert all(not torch.equal(before[k], v) for k, v in ppo.policy.state_dict().items())   # every tensor, the conv's included
    assert all(math.isfinite(l[k]) for l in logs for k in STAT_KEYS)
    _check_head(vec, ppo)
    vec.close()


@pytest.mark.gpu
def test_captured_hip_cnn_update_matches_the_torch_graph_on_gpu():
    from gym_fixed_wing import presets
    from gym_fixed_wing.vec_env import FixedWingVecEnv

    def make():   # (the build-time cnn preset, as examples/train_ppo.py --policy cnn makes it: nothing to compile)
        vec = FixedWingVecEnv(presets.preset("cnn"), num_envs=4096, derived_views=True, seed=3, device=0)
        vec.set_curriculum_level(0.25)
        vec.reset()
        return vec
    vec, ph, batch = _check_composed(make)
    assert ph.learner._graph is not None     # the update ran as a captured graph
    _check_head(vec, ph)
    vec.close()


# ---- refusals, lifecycle -----------------------------------------------------------------------------------------------------
def test_cnn_learner_refusals_emulated():
    lib, mem = _emu()
    mlp = DeviceActor(64, D, _backend=mem, _lib=lib)
    h = ctypes.c_void_p()
    assert lib.fwg_learner_create_cnn(mlp._handle, ctypes.byref(h)) != 0 and not h.value
    assert b"fwg_learner_create" in lib.fwg_last_error().replace(b"fwg_learner_create_cnn", b"")
    assert lib.fwg_learner_create_cnn(None, ctypes.byref(h)) != 0 and b"null" in lib.fwg_last_error()
    assert lib.fwg_learner_create_cnn(mlp._handle, None) != 0 and b"null" in lib.fwg_last_error()
    cnn = DeviceActor(64, D, _backend=mem, _lib=lib)
    cnn.load_policy(CnnMlpPolicy())
    assert lib.fwg_learner_create(cnn._handle, ctypes.byref(h)) != 0
    assert b"conv" in lib.fwg_last_error() and b"fwg_learner_create_cnn" in lib.fwg_last_error()
    # a head changed back to the MLP under a CNN learner: the pack refuses instead of writing another layout
    L = HipLearner(lib, cnn, CnnMlpPolicy(), CPU, graph=False)
    nat.check(lib, lib.fwg_actor_set_conv(cnn._handle, 0, 0, None, None))
    with pytest.raises(nat.NativeError, match="fwg_actor_pack"):
        L.pack()
    # a policy of another layout than the learner's
    cnn.load_policy(CnnMlpPolicy())
    with pytest.raises(ValueError, match="parameters"):
        HipLearner(lib, cnn, MlpPolicy(D), CPU, graph=False)
    del L
    mlp.close(), cnn.close()


def test_ppo_update_strings():
    with pytest.raises(ValueError, match="conv"):
        PPO(object(), policy=MlpPolicy(12), update="hip_cnn")
    with pytest.raises(ValueError, match="conv"):
        PPO(object(), policy=None, update="hip_cnn")
    with pytest.raises(ValueError, match="hip_cnn"):
        PPO(object(), policy=CnnMlpPolicy(), update="hip")
    with pytest.raises(ValueError):
        PPO(object(), policy=CnnMlpPolicy(), update="jax")


def test_train_ppo_selects_the_cnn_learner_emulated(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_ppo
    monkeypatch.setattr(train_ppo, "make_sharded_env", lambda *a, **kw: _emu_vec())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    ppo, res = train_ppo.train(envs=70, timesteps=16 * 70, seed=0, nminibatches=4, noptepochs=1, n_steps=16, log=None,
                               policy="cnn", update="hip")
    assert isinstance(ppo.learner, HipLearner) and ppo.learner.num_params == 13337 and res["updates"] == 1
    ppo.vec.close()


def test_cnn_learner_create_frees_what_it_allocated():
    from test_host_lifecycle import _check_create
    lib, mem = _emu()
    head = DeviceActor(70, D, _backend=mem, _lib=lib)
    head.load_policy(CnnMlpPolicy())
    k_allocs = _check_create(lib, lambda out: lib.fwg_learner_create_cnn(head._handle, ctypes.byref(out)), lib.fwg_learner_destroy)
    assert k_allocs == 2   # partial-gradient slab, flat gradient
    head.close()


# ---- the build's resource report ---------------------------------------------------------------------------------------------
def test_cnn_gradient_kernel_has_no_scratch_and_no_spills():
    with open(specialize.RESOURCES_JSON) as f:
        rep = json.load(f)["kernels"]
    grads = {k: v for k, v in rep.items() if re.match(r"^void k_ppo_grad<", k)}
    cnn = [v for k, v in grads.items() if k.startswith("void k_ppo_grad<true>")]
    assert len(cnn) == 1, sorted(grads)
    assert cnn[0]["ScratchSize [bytes/lane]"] == 0 and cnn[0]["VGPRs Spill"] == 0, cnn[0]
