"""The CNN controller on the MI355X: the HIP head's conv front end (k_actor_act_cnn) against torch fp32 CnnMlpPolicy at 65 536
envs of the cnn preset (row log read in place and the dense batch), the shipped controller (tests/golden/cnn_controller.npz)
flying the 100 shipped no-wind scenarios through the reference's evaluation protocol, and a short PPO run from scratch.
This file keeps the large batch and the closed loop; the head's arithmetic per element against float64 -- tile tails, act_dim 1..4,
the single-product instance, the row log across wraps, clipping, the noise stream, capture -- is pinned by
tests/test_actor_contract_cnn.py."""
import json
import os
import time

import numpy as np
import pytest
import torch

import configs
from gym_fixed_wing import evaluate as ev
from gym_fixed_wing.actor import DeviceActor, load_controller, module_from_weights, weights_from_stable_baselines
from gym_fixed_wing.rollout import CnnMlpPolicy
from gym_fixed_wing.vec_env import FixedWingVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
    return load_controller(os.path.join(HERE, "golden", "cnn_controller.npz"))


@pytest.mark.gpu
def test_cnn_head_matches_torch_on_gpu():
    n = 65536
    m = _fixture()
    vec = FixedWingVecEnv(configs.reference_like("cnn"), num_envs=n, device=0, config_kw={"observation": {"step": 2}, "steps_max": 60},
                          sim_config_kw={"turbulence": True, "turbulence_intensity": "moderate"}, seed=2, derived_views=False)
    assert vec.obs_log_rows > 0 and vec.obs_shape == (5, 12)
    vec.reset()
    torch.manual_seed(4)
    pol = CnnMlpPolicy()
    with torch.no_grad():
        pol.conv.weight.normal_(0.0, 0.8)
        for p in list(pol.pi) + list(pol.vf):
            if isinstance(p, torch.nn.Linear):
                p.weight.mul_(2.5)
    pol = pol.cuda()
    heads = {}
    for layout in ("log", "dense"):
        for training in (True, False):
            a = DeviceActor.for_env(vec, seed=3, training=training)
            a.load_policy(pol)
            if not training:
                a.set_stats(np.asarray(m["obs_rms"]["mean"]).reshape(-1), np.asarray(m["obs_rms"]["var"]).reshape(-1), 1e6)
            if layout == "log":
                a.set_obs_log(vec)
            heads[(layout, training)] = a
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    worst = {}
    for t in range(12):
        o, r, d = vec.step_device(torch.rand((n, 3), device="cuda", generator=gen) * 2 - 1)
        if t % 3 != 2:
            continue
        dense = o.contiguous().reshape(n, -1)
        out = {}
        for (layout, training), a in heads.items():
            src = vec._obs_buf if layout == "log" else dense
            if training:
                a.observe(src)
            no, mean, val, _, _ = a.act(src, deterministic=True)
            out[(layout, training)] = (no.clone(), mean.clone(), val.clone())
            with torch.no_grad():
                w_mean, w_val = pol.pi(no), pol.vf(no).squeeze(-1)
            key = "{}_{}".format(layout, "train" if training else "frozen")
            e = max(float((mean - w_mean).abs().max() / w_mean.abs().max()), float((val - w_val).abs().max() / w_val.abs().max()))
            worst[key] = max(worst.get(key, 0.0), e)
        for training in (True, False):   # the two layouts: the same head on the same numbers
            for x, y in zip(out[("log", training)], out[("dense", training)]):
                assert torch.equal(x, y), (t, training)
    print("CNN head vs torch fp32, 65 536 envs:", worst)
    assert max(worst.values()) < 2e-5, worst
    for a in heads.values():
        a.close()
    vec.close()


def _scenarios():
    with open(os.path.join(HERE, "golden", "test_set_wind_none.json")) as f:
        return json.load(f)


@pytest.mark.gpu
def test_shipped_cnn_controller_flies_the_shipped_test_set():
    m = _fixture()
    z = np.load(os.path.join(HERE, "golden", "eval_res_RL_CNN_none_rewards.npz"))   # first 100 steps, NaN past an episode's end
    pub = {"rewards": [r[:min(int(n), r.size)].astype(np.float64) for r, n in zip(z["rewards"], z["episode_lengths"])]}
    scen = _scenarios()
    w = weights_from_stable_baselines(m["weights"])
    actor = DeviceActor(len(scen), 60, training=False, device=0)
    actor.load_policy(w)
    actor.set_stats(np.asarray(m["obs_rms"]["mean"]).reshape(-1), np.asarray(m["obs_rms"]["var"]).reshape(-1), 1e6)
    raw = module_from_weights(w, (5, 12)).cuda()

    def first_step(obs):   # evaluate_controller.py:118: the first action of an episode sees the UN-normalised observation
        with torch.no_grad():
            return raw.pi(obs.reshape(obs.shape[0], -1))

    res = ev.evaluate_on_set(scen, configs.reference_like("cnn"), device=0, first_step_policy=first_step,
                             policy=lambda obs: actor.act(obs.reshape(obs.shape[0], -1).contiguous(), deterministic=True)[1])
    table = ev.summarize(res)
    dm = np.concatenate([np.abs(np.array(a[:min(len(a), len(b))]) - np.array(b[:min(len(a), len(b))]))
                         for a, b in zip(res["rewards"], pub["rewards"])])
    second = float(np.mean([abs(a[1] - b[1]) for a, b in zip(res["rewards"], pub["rewards"])]))
    report = {"ours": table, "mean_abs_dreward_first100": float(dm.mean()), "p90_abs_dreward_first100": float(np.percentile(dm, 90)),
              "second_step_reward_abs_err": second,
              "published_README_RL_CNN_none": {"success_%": 100, "settling_time": [1.594, 1.580, 2.704], "control_variation": 0.638}}
    print(json.dumps(report, indent=1))
    # GATES (float64 oracle, tools/cnn_trace.py on all 100: success 96 %, |dr| 0.0172 / p90 0.036, second step 0.0005, cv 0.605)
    assert min(table["success_%"].values()) >= 95.0, table["success_%"]   # published 100/100/100/100
    assert dm.mean() < 0.022 and np.percentile(dm, 90) < 0.045, (dm.mean(), np.percentile(dm, 90))
    assert second < 2e-3, second
    assert abs(table["control_variation"]["all"] - 0.638) <= 0.30 * 0.638, table["control_variation"]
    actor.close()


@pytest.mark.gpu
def test_short_cnn_training_run_learns():
    """PPO with CnnMlpPolicy from random initialisation on 4 096 envs of the cnn preset with the curriculum (the reference's
    --policy CNN recipe; examples/train_ppo.py --policy cnn).  Gate: the success rate of the last cohort of finished episodes
    beats the first one's by 0.03, or the curriculum was raised.  Measured on the MI355X: 62 updates in 34 s, cohorts
    0.001 -> 0.094 -> 0.983 (a gate of +0.03 leaves a margin of 30x; an earlier 24 M-step run: 0.001 -> 0.069)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
    import train_ppo
    hist = []
    t0 = time.perf_counter()
    ppo, res = train_ppo.train(envs=4096, timesteps=32e6, seed=0, policy="cnn", log=None,
                               on_update=lambda p, info: hist.append(info))
    dt = time.perf_counter() - t0
    cohorts = [(h["success"]["all"], h["level"]) for h in hist if h["episodes"] > 0]
    print("CNN training: {:.1f} s, {} updates, {:.3e} steps/s; success per cohort {}".format(
        dt, ppo.updates, res["env_steps_per_s"], [round(c[0], 3) for c in cohorts]))
    assert ppo.actor.cnn
    assert len(cohorts) >= 2
    assert cohorts[-1][0] > cohorts[0][0] + 0.03 or max(c[1] for c in cohorts) > cohorts[0][1], cohorts
    assert dt < 60
