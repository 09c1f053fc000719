"""The CNN controller (the reference's CnnMlpPolicy: examples/train_rl_controller.py:179-197 --policy CNN, shipped as
examples/models/cnn_controller -> tests/golden/cnn_controller.npz): the fixture, the torch policy, the HIP head's conv front end
(fwg_actor_set_conv; CPU: the host-emulation build of the kernels) against a float64 numpy forward, the (A, F) choice against the
published closed-loop rewards on the float64 oracle, the torch PPO step and the refusals."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from gym_fixed_wing import _native as nat
from gym_fixed_wing.actor import DeviceActor, load_controller, module_from_weights, weights_from_module, weights_from_stable_baselines
from gym_fixed_wing.rollout import CNN_ACTIVATION, CNN_FLATTEN, CnnMlpPolicy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ACTS = {"identity": lambda z: z, "tanh": np.tanh, "relu": lambda z: np.maximum(z, 0.0)}


def _fixture():
    return load_controller(os.path.join(HERE, "golden", "cnn_controller.npz"))


def np_forward(w, x, act=CNN_ACTIVATION, order=CNN_FLATTEN):
    """float64 CnnMlpPolicy on normalised observations x [N, rows * features]; w in torch layout (weights_from_*)."""
    cw = np.asarray(w["c1_w"], np.float64)
    rows, nf = cw.shape
    X = np.asarray(x, np.float64).reshape(len(x), rows, -1)
    y = ACTS[act](np.einsum("nrj,rc->njc", X, cw) + np.asarray(w["c1_b"], np.float64))
    feat = y.reshape(len(x), -1) if order == "nhwc" else y.transpose(0, 2, 1).reshape(len(x), -1)
    out = []
    for net in ("pi", "vf"):
        h = np.tanh(feat @ np.asarray(w[net + "_w0"], np.float64).T + np.asarray(w[net + "_b0"], np.float64))
        h = np.tanh(h @ np.asarray(w[net + "_w1"], np.float64).T + np.asarray(w[net + "_b1"], np.float64))
        out.append(h @ np.asarray(w[net + "_w2"], np.float64).T + np.asarray(w[net + "_b2"], np.float64))
    return out[0], out[1][:, 0]


def _random_policy(seed):
    torch.manual_seed(seed)
    pol = CnnMlpPolicy((5, 12), n_filters=3)
    with torch.no_grad():
        pol.conv.weight.normal_(0.0, 0.8)
        pol.conv.bias.normal_(0.0, 0.5)
        pol.log_std.copy_(torch.tensor([-0.3, 0.1, 0.4]))
        for m in list(pol.pi) + list(pol.vf):
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(2.5)   # larger pre-activations: tanh away from its linear range
    return pol


# ----------------------------------------------------------------------------------------------------------------------
# fixture, torch policy
# ----------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_checkpoint():
    z = np.load(os.path.join(HERE, "golden", "cnn_controller.npz"))
    s = {k[2:]: z[k].shape for k in z.files if k.startswith("w_")}
    assert s["c1_w"] == (5, 1, 1, 3) and s["c1_b"] == (1, 3, 1, 1)
    assert s["pi_fc0_w"] == (36, 64) and s["vf_fc0_w"] == (36, 64) and s["pi_fc1_w"] == (64, 64) and s["vf_fc1_w"] == (64, 64)
    assert s["pi_w"] == (64, 3) and s["vf_w"] == (64, 1) and s["pi_logstd"] == (1, 3)
    assert "q_w" not in s
    assert int(z["n_filters"]) == 3 and z["observation_shape"].tolist() == [5, 12]
    hp = {k[5:]: z[k].item() for k in z.files if k.startswith("ppo2_")}
    assert (hp["n_steps"], hp["nminibatches"], hp["noptepochs"], hp["n_envs"], hp["num_timesteps"]) == (128, 4, 4, 6, 3218320)
    assert (hp["cliprange"], hp["ent_coef"], hp["vf_coef"], hp["max_grad_norm"]) == (0.2, 0.01, 0.5, 0.5)
    assert z["obs_rms_mean"].shape == (5, 12) and z["obs_rms_var"].shape == (5, 12)
    assert 3.0e6 < float(z["obs_rms_count"]) < 3.3e6
    assert z["ret_rms_var"].shape == () and float(z["ret_rms_var"]) > 0
    pub = np.load(os.path.join(HERE, "golden", "eval_res_RL_CNN_none_rewards.npz"))
    assert pub["rewards"].shape == (100, 100) and float(pub["success_all"]) == 100.0
    assert abs(float(pub["control_variation"]) - 0.638) < 1e-3


def test_torch_policy_matches_float64_forward():
    pol = _random_policy(3)
    w = weights_from_module(pol)
    assert w["c1_w"].shape == (5, 3) and w["pi_w0"].shape == (64, 36)
    x = np.random.default_rng(0).normal(size=(300, 60)) * 2
    with torch.no_grad():
        t = torch.from_numpy(x).double()
        mean, val = pol.double().pi(t).numpy(), pol.vf(t).squeeze(-1).numpy()
        mean3 = pol.pi(t.reshape(300, 5, 12)).numpy()   # matrix-shaped input too
    m64, v64 = np_forward(w, x)
    np.testing.assert_allclose(mean, m64, atol=1e-6)
    np.testing.assert_allclose(val, v64, atol=1e-6)
    np.testing.assert_array_equal(mean, mean3)
    # the conv is ONE module shared by pi and vf
    assert pol.pi[0] is pol.vf[0] is pol.conv
    assert sum(p.numel() for p in pol.parameters()) == 15 + 3 + 2 * (36 * 64 + 64 + 64 * 64 + 64) + 64 * 3 + 3 + 64 + 1 + 3


def test_torch_policy_matches_float64_forward_on_the_shipped_weights():
    m = _fixture()
    w = weights_from_stable_baselines(m["weights"])
    assert w["c1_w"].shape == (5, 3) and w["c1_b"].shape == (3,) and w["log_std"].shape == (3,)
    np.testing.assert_array_equal(w["c1_w"], np.asarray(m["weights"]["c1_w"], np.float32)[:, 0, 0, :])
    pol = module_from_weights(w).double()
    x = np.clip(np.random.default_rng(1).normal(size=(200, 60)) * 1.5, -10, 10)
    with torch.no_grad():
        mean = pol.pi(torch.from_numpy(x)).numpy()
    # TF layout straight from the fixture ([in][out] kernels), float64
    W = {k: np.asarray(v, np.float64) for k, v in m["weights"].items()}
    y = np.tanh(np.einsum("nrj,rc->njc", x.reshape(200, 5, 12), W["c1_w"][:, 0, 0, :]) + W["c1_b"].reshape(-1)).reshape(200, 36)
    h = np.tanh(np.tanh(y @ W["pi_fc0_w"] + W["pi_fc0_b"]) @ W["pi_fc1_w"] + W["pi_fc1_b"])
    np.testing.assert_allclose(mean, h @ W["pi_w"] + W["pi_b"], atol=1e-6)


# ----------------------------------------------------------------------------------------------------------------------
# the HIP head's CNN front end (host emulation of k_actor_act_cnn)
# ----------------------------------------------------------------------------------------------------------------------
def _emu():
    from emu.host_backend import HostBackend, build_emu
    return dict(_backend=HostBackend(), _lib=nat.load_library(build_emu()))


class _Rms64(object):
    def __init__(self, d):
        self.mean, self.var, self.count = np.zeros(d), np.ones(d), 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        bm, bv, bc = x.mean(axis=0), x.var(axis=0), x.shape[0]
        delta, tot = bm - self.mean, self.count + bc
        m2 = self.var * self.count + bv * bc + delta ** 2 * self.count * bc / tot
        self.mean, self.var, self.count = self.mean + delta * bc / tot, m2 / tot, tot


def _obs_source(layout, n, seed):
    """-> (next_batch() -> (head input, dense float64 [n][60]), keep-alive).  dense: random batches; log: a 5 x 12 row-log env
    (the cnn preset) stepped under random actions, the head reading its window in place."""
    rng = np.random.default_rng(seed)
    if layout == "dense":
        scale, shift = rng.uniform(0.5, 4.0, 60), rng.uniform(-5, 5, 60)

        def nxt():
            x = (rng.normal(size=(n, 60)) * scale + shift).astype(np.float32)
            return x, x.astype(np.float64)
        return nxt, None
    import configs
    from emu.host_backend import HostBackend, build_emu
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    vec = FixedWingVecEnv(configs.reference_like("cnn"), num_envs=n, config_kw={"observation": {"step": 2}, "steps_max": 40},
                          as_numpy=True, _backend=HostBackend(), _lib_path=build_emu(), obs_log_rows=10, seed=seed)
    assert vec.obs_log_rows > 0 and vec.obs_shape == (5, 12)
    vec.reset()

    def nxt():
        o, _, _, _ = vec.step(rng.uniform(-1, 1, size=(n, 3)).astype(np.float32))
        return vec._obs_buf, np.asarray(o, np.float64).reshape(n, 60)
    return nxt, vec


def run_cnn_head(layout, training, n=256, steps=3, wrong=None):
    """Head outputs against the float64 forward; returns the worst relative errors.  wrong=(A, F): score the head against
    that reading instead of the frozen one."""
    pol = _random_policy(5)
    w = weights_from_module(pol)
    m = _fixture()
    actor = DeviceActor(n, 60, seed=11, env_id_base=3, training=training, **_emu())
    actor.load_policy(pol)
    assert actor.cnn
    nxt, vec = _obs_source(layout, n, 7)
    if vec is not None:
        actor.set_obs_log(vec)
    rms = _Rms64(60)
    if not training:
        mean0, var0 = np.asarray(m["obs_rms"]["mean"]).reshape(-1), np.asarray(m["obs_rms"]["var"]).reshape(-1)
        actor.set_stats(mean0, var0, 1e6)
        rms.mean, rms.var = mean0.astype(np.float32).astype(np.float64), var0.astype(np.float32).astype(np.float64)
    mem = actor._mem
    act_f, order_f = wrong or (CNN_ACTIVATION, CNN_FLATTEN)
    worst = {"obs": 0.0, "mean": 0.0, "value": 0.0, "logp": 0.0}
    for t in range(steps):
        src, x64 = nxt()
        src_d = mem.from_host(src) if layout == "dense" else src
        if training:
            actor.observe(src_d)
            rms.update(x64)
        no, mean, val, _, _ = actor.act(src_d, deterministic=True)
        want_no = np.clip((x64 - rms.mean) / np.sqrt(rms.var + 1e-8), -10, 10)
        no = np.asarray(no, np.float64)
        # (relative above 1: fp32 statistics of env observations whose first batches barely vary)
        worst["obs"] = max(worst["obs"], float((np.abs(no - want_no) / np.maximum(1.0, np.abs(want_no))).max()))
        m64, v64 = np_forward(w, no, act_f, order_f)   # the networks on the head's own normalised observation
        worst["mean"] = max(worst["mean"], float(np.abs(np.asarray(mean) - m64).max() / np.abs(m64).max()))
        worst["value"] = max(worst["value"], float(np.abs(np.asarray(val) - v64).max() / np.abs(v64).max()))
        _, a, _, lp, _ = actor.act(src_d)   # sampled (no new moments: same statistics): logp of the drawn noise, seed fixed
        ls = pol.log_std.detach().numpy().astype(np.float64)
        z = (np.asarray(a, np.float64) - m64) / np.exp(ls)
        want_lp = (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(axis=1)
        worst["logp"] = max(worst["logp"], float(np.abs(np.asarray(lp) - want_lp).max()))
        if wrong is None:
            assert np.abs(np.asarray(a) - np.asarray(mean)).max() > 0.05   # really sampled
    st = actor.get_stats()
    if training:
        np.testing.assert_allclose(st["obs_mean"], rms.mean, rtol=2e-5, atol=2e-5)
    else:
        np.testing.assert_allclose(st["obs_mean"], rms.mean, rtol=1e-6)   # frozen
    actor.close()
    if vec is not None:
        vec.close()
    return worst


@pytest.mark.parametrize("layout", ["dense", "log"])
@pytest.mark.parametrize("training", [True, False])
def test_emulated_cnn_head_matches_float64_forward(layout, training):
    w = run_cnn_head(layout, training)
    print(layout, training, w)
    # normalised observation: the head's fp32 running statistics (the MLP head's code, unchanged) against float64 -- env
    # observations of a few steps have means ~20 over variances ~1e-2, so the bar is relative (measured 7e-5 on the row log)
    assert w["obs"] < 2e-4, w
    assert w["mean"] < 2e-5 and w["value"] < 2e-5, w   # the MLP head's bar
    assert w["logp"] < 2e-3, w   # (noise through the action: z = (a - mean) / std, a ~ 1)


@pytest.mark.parametrize("wrong", [("identity", "nhwc"), ("relu", "nhwc"), ("tanh", "chw")])
def test_a_head_wired_to_another_reading_fails_the_comparison(wrong):
    w = run_cnn_head("dense", False, n=64, steps=1, wrong=wrong)
    assert w["mean"] > 1e-2 and w["value"] > 1e-2, (wrong, w)


# ----------------------------------------------------------------------------------------------------------------------
# the (A, F) choice on the float64 oracle (tools/cnn_trace.py; profiles/cnn_architecture.txt)
# ----------------------------------------------------------------------------------------------------------------------
N_SCEN = 20


def _fly_all(cands, max_steps):
    import multiprocessing as mp
    import tempfile
    import configs
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cnn_trace as ct
    cfg = configs.reference_like("cnn")
    with open(os.path.join(HERE, "golden", "test_set_wind_none.json")) as f:
        scen = json.load(f)[:N_SCEN]
    tmpdir = tempfile.mkdtemp()
    jobs = [(c, sc, cfg, tmpdir, max_steps) for c in cands for sc in scen]
    with mp.get_context("fork").Pool(max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        res = pool.map(ct.fly, jobs, chunksize=1)
    return {c: res[i * N_SCEN:(i + 1) * N_SCEN] for i, c in enumerate(cands)}


def _dr(res, pub):
    """(mean |reward - published| over the first 100 steps, |error| of the second step's reward -- the first action on a
    normalised observation) over the scenarios flown."""
    d = np.concatenate([np.abs(np.array(a[:min(len(a), len(b), 100)]) - np.array(b[:min(len(a), len(b), 100)]))
                        for (a, _), b in zip(res, pub["rewards"])])
    return float(d.mean()), float(np.mean([abs(a[1] - b[1]) for (a, _), b in zip(res, pub["rewards"])]))


# Bounds from tools/cnn_trace.py's numbers.  All 100 scenarios (profiles/cnn_architecture.txt): the frozen reading 96 % success,
# |dr| 0.0172, second-step error 0.0005; the next best (identity, nhwc) 87 %, 0.0281, 0.0193.  The first 20 scenarios, first 100
# steps (measured): tanh/nhwc |dr| 0.0278 against 0.0354 (identity/nhwc), 0.0364 (relu/nhwc), 0.36-0.40 (the filter-major three).
DR_MAX, SECOND_MAX = 0.031, 2e-3


def test_shipped_cnn_controller_flies_on_the_float64_oracle_and_only_the_frozen_reading_does():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cnn_trace
    pub = cnn_trace.published()
    frozen = (CNN_ACTIVATION, CNN_FLATTEN)
    others = [(a, o) for o in ("nhwc", "chw") for a in ACTS if (a, o) != frozen]
    full = _fly_all([frozen], None)[frozen]
    ok = [bool(i["success"]["all"]) for _, i in full]
    dr, second = _dr(full, pub)
    print("frozen {}: success {}/{}, mean |dr| first 100 steps {:.4f}, second step {:.5f}".format(frozen, sum(ok), len(ok), dr, second))
    assert sum(ok) >= 18            # measured 20/20 (published 100 %)
    assert dr < DR_MAX and second < SECOND_MAX
    # the rejected readings, first 100 steps: every one misses the bounds
    for c, res in _fly_all(others, 100).items():
        d, s2 = _dr(res, pub)
        print("rejected {}: mean |dr| {:.4f}, second step {:.5f}".format(c, d, s2))
        assert d > DR_MAX and s2 > SECOND_MAX, (c, d, s2)


# ----------------------------------------------------------------------------------------------------------------------
# training: the torch PPO step; the refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_ppo_minibatch_gradients_of_the_conv_equal_float64_autograd():
    from gym_fixed_wing.ppo import ppo_loss, sb_init_
    torch.manual_seed(0)
    pol = sb_init_(CnnMlpPolicy())
    w = pol.conv.weight.detach().numpy()
    np.testing.assert_allclose(w.T @ w, 2.0 * np.eye(3), atol=1e-5)   # orthogonal columns, gain sqrt(2)
    assert float(pol.conv.bias.detach().abs().sum()) == 0.0
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    rng = np.random.default_rng(2)
    mb = 64
    batch = {"obs": rng.normal(size=(mb, 60)), "actions": rng.normal(size=(mb, 3)), "values": rng.normal(size=mb),
             "logp": rng.normal(size=mb) - 3, "adv": rng.normal(size=mb), "returns": rng.normal(size=mb)}
    grads = []
    for dt in (torch.float32, torch.float64):
        p = CnnMlpPolicy().to(dt)
        p.load_state_dict({k: v.to(dt) for k, v in pol.state_dict().items()})
        b = {k: torch.as_tensor(v, dtype=dt) for k, v in batch.items()}
        loss, _ = ppo_loss(p, b["obs"], b["actions"], b["values"], b["logp"], b["adv"], b["returns"], 0.2, 0.01, 0.5)
        loss.backward()
        grads.append((p.conv.weight.grad.double().numpy(), p.conv.bias.grad.double().numpy()))
    assert np.abs(grads[1][0]).max() > 1e-4
    np.testing.assert_allclose(grads[0][0], grads[1][0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(grads[0][1], grads[1][1], rtol=1e-4, atol=1e-6)


def test_hip_update_with_a_cnn_policy_raises():
    from gym_fixed_wing.ppo import PPO
    with pytest.raises(ValueError, match="conv"):
        PPO(object(), policy=CnnMlpPolicy(), update="hip")


def test_set_conv_refuses_bad_shapes():
    kw = _emu()
    lib = kw["_lib"]
    w, b = np.zeros((8, 8), np.float32), np.zeros(8, np.float32)
    a = DeviceActor(64, 60, **kw)
    h = a._handle
    for nf, rows, what in ((3, 7, b"matrix"), (3, 1, b"matrix"), (6, 5, b"64"), (3, 4, b"5 x 12"), (2, 5, b"5 x 12")):
        assert lib.fwg_actor_set_conv(h, nf, rows, w.ctypes.data, b.ctypes.data) != 0, (nf, rows)
        assert what in lib.fwg_last_error(), (nf, rows, lib.fwg_last_error())
    v = DeviceActor(64, 12, **_emu())   # a vector observation: no window to convolve
    assert lib.fwg_actor_set_conv(v._handle, 3, 5, w.ctypes.data, b.ctypes.data) != 0
    assert b"matrix" in lib.fwg_last_error()
    assert lib.fwg_actor_set_conv(h, 3, 5, w.ctypes.data, b.ctypes.data) == 0
    assert lib.fwg_actor_set_conv(h, 0, 0, None, None) == 0   # back to the MLP
    with pytest.raises(ValueError, match="pi_w0"):   # the MLP head refuses 36-input weights and vice versa
        a.load_policy({k: v for k, v in weights_from_module(CnnMlpPolicy()).items() if not k.startswith("c1_")})
    # a CNN head is not for the one-launch step nor for the HIP learner
    a.load_policy(CnnMlpPolicy())
    L = ctypes.c_void_p()
    assert lib.fwg_learner_create(h, ctypes.byref(L)) != 0 and b"conv" in lib.fwg_last_error()
    a.close(), v.close()


def test_rows_other_than_the_observation_length_are_refused_on_a_row_log():
    import configs
    from emu.host_backend import HostBackend, build_emu
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    vec = FixedWingVecEnv(configs.reference_like("cnn"), num_envs=32, config_kw={"observation": {"step": 2}}, as_numpy=True,
                          _backend=HostBackend(), _lib_path=build_emu(), obs_log_rows=10, seed=1)
    a = DeviceActor.for_env(vec)
    a.set_obs_log(vec)
    lib = vec._lib
    w, b = np.zeros(64, np.float32), np.zeros(8, np.float32)
    assert lib.fwg_actor_set_conv(a._handle, 3, 6, w.ctypes.data, b.ctypes.data) != 0
    assert lib.fwg_actor_set_conv(a._handle, 3, 4, w.ctypes.data, b.ctypes.data) != 0
    assert b"observation length" in lib.fwg_last_error()
    a.load_policy(CnnMlpPolicy())
    assert a.cnn
    a.close(), vec.close()
