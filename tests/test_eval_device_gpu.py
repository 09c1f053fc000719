"""The evaluation protocol on the device, GPU half (the CPU half and the description of the shared pieces:
tests/test_eval_device.py, tests/eval_device_common.py).

  kernels      fwg_eval_advance against the numpy restatement (exact) and fwg_pid_act against float64, the shapes and bounds of
               the CPU half, on the MI355X;
  head path    65 shipped scenarios (a full wave plus one lane) through evaluate_on_set_device with the shipped MLP / CNN
               controller in the HIP rollout head: rewards, lengths, terminations and the five metrics BIT-IDENTICAL to
               evaluate_on_set driven by the same head (same kernels, same inputs, independent lanes), calm and in turbulence;
  PID path     against the host loop's BatchedPID (torch arithmetic) within the bands tests/test_evaluate.py applies between two
               arithmetic paths of one controller;
  PPO.evaluate leaves the training run bit for bit where it was; train_ppo's --test-set evaluates four times in a run."""
import json
import os
import sys

import numpy as np
import pytest

import configs
import eval_device_common as edc
from gym_fixed_wing import _native as nat
from gym_fixed_wing import evaluate as ev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_SCEN = 65      # a full wave plus one lane


def _scenarios(n=N_SCEN):
    with open(os.path.join(HERE, "golden", "test_set_wind_none.json")) as f:
        return json.load(f)[:n]


@pytest.fixture(scope="module")
def gpu():
    from gym_fixed_wing.vec_env import _TorchBackend
    return nat.load_library(), _TorchBackend(0)


@pytest.mark.parametrize("n", edc.TRACKER_N)
def test_tracker_matches_the_numpy_restatement_exactly(gpu, n):
    got, want, sentinels = edc.run_tracker(*gpu, n)
    edc.assert_tracker(got, want, sentinels)


def test_tracker_and_pid_refuse_bad_arguments(gpu):
    for out in (edc.tracker_refusals(*gpu), edc.pid_refusals(*gpu)):
        for name, (status, msg) in out.items():
            assert status == -1, name
            assert msg.startswith("fwg_"), (name, msg)


@pytest.mark.parametrize("n", edc.PID_N)
def test_pid_head_against_float64(gpu, n):
    acts, integ, inp = edc.run_pid(*gpu, n)
    edc.assert_pid_inputs_exercise_every_term(inp)
    err = edc.pid_errors(acts, integ, inp)
    print("fwg_pid_act on the GPU, N = {}: {}".format(n, {k: "%.3g" % v for k, v in err.items()}))
    assert edc.PID_BOUND <= 1e-3
    for k, v in err.items():
        assert v <= edc.PID_BOUND, (k, v, edc.PID_BOUND)


# ------------------------------------------------------------------------------------------------------------- head path
def _mlp_head(n):
    import torch
    from gym_fixed_wing.actor import DeviceActor, weights_from_stable_baselines
    with open(os.path.join(HERE, "golden", "mlp_controller.json")) as f:
        m = json.load(f)
    W = {k: torch.tensor(v, dtype=torch.float32, device="cuda") for k, v in m["weights"].items()}

    def raw_policy(x):   # the first action of an episode: the network on the UN-normalised reset observation
        h = torch.tanh(x.reshape(x.shape[0], -1) @ W["pi_fc0_w"] + W["pi_fc0_b"])
        h = torch.tanh(h @ W["pi_fc1_w"] + W["pi_fc1_b"])
        return h @ W["pi_w"] + W["pi_b"]
    actor = DeviceActor(n, 12, training=False, device=0)
    actor.load_policy(weights_from_stable_baselines(m["weights"]))
    actor.set_stats(m["obs_rms"]["mean"], m["obs_rms"]["var"], 1e6)
    return actor, raw_policy


def _cnn_head(n):
    from gym_fixed_wing.actor import DeviceActor, load_controller, module_from_weights, weights_from_stable_baselines
    m = load_controller(os.path.join(HERE, "golden", "cnn_controller.npz"))
    w = weights_from_stable_baselines(m["weights"])
    mean, var = np.asarray(m["obs_rms"]["mean"]), np.asarray(m["obs_rms"]["var"])
    actor = DeviceActor(n, int(mean.size), training=False, device=0)
    actor.load_policy(w)
    actor.set_stats(mean.reshape(-1), var.reshape(-1), 1e6)
    net = module_from_weights(w, mean.shape).to("cuda:0")
    return actor, lambda obs: net.pi(obs.reshape(obs.shape[0], -1))


def _assert_same_bits(result, host):
    res = result.as_reference_layout()
    assert set(res) == set(host)
    assert res["termination"] == host["termination"]
    assert [len(r) for r in res["rewards"]] == [len(r) for r in host["rewards"]] == [int(x) for x in result.length]
    for i, (a, b) in enumerate(zip(res["rewards"], host["rewards"])):
        assert np.array(a, dtype=np.float64).tobytes() == np.array(b, dtype=np.float64).tobytes(), i
    for m in ev.METRICS:
        assert set(res[m]) == set(host[m]) and len(res[m]) > 0, m
        for state in res[m]:
            a, b = res[m][state], host[m][state]
            assert [type(x) for x in a] == [type(x) for x in b], (m, state)
            assert np.array(a, dtype=np.float64).tobytes() == np.array(b, dtype=np.float64).tobytes(), (m, state)   # (None -> NaN on both sides)
    np.testing.assert_equal(result.table(), ev.summarize(res))
    np.testing.assert_equal(result.table(), ev.summarize(host))


@pytest.mark.parametrize("kind,turbulence,seed", [("mlp", "none", 0), ("mlp", "light", 1), ("cnn", "none", 0)])
def test_head_path_is_bit_identical_to_the_host_loop(kind, turbulence, seed):
    scen = _scenarios()
    actor, first = (_mlp_head if kind == "mlp" else _cnn_head)(len(scen))
    cfg = configs.reference_like(kind)
    host = ev.evaluate_on_set(scen, cfg, policy=lambda obs: actor.act(obs.reshape(obs.shape[0], -1).contiguous(), deterministic=True)[1],
                              first_step_policy=first, device=0, seed=seed, turbulence_intensity=turbulence)
    result = ev.evaluate_on_set_device(scen, cfg, controller=actor, first_step_policy=first, device=0, seed=seed,
                                       turbulence_intensity=turbulence)
    assert sum(t is not None for t in host["termination"]) >= 60       # the comparison is about finished episodes
    _assert_same_bits(result, host)
    actor.close()


# -------------------------------------------------------------------------------------------------------------- PID path
def test_pid_path_against_the_host_loop():
    scen, cfg = _scenarios(), configs.reference_like("examples")
    host = ev.evaluate_on_set(scen, cfg, device=0)
    result = ev.evaluate_on_set_device(scen, cfg, device=0)
    res, table, table_host = result.as_reference_layout(), result.table(), ev.summarize(host)
    lengths, lengths_host = np.array([len(r) for r in res["rewards"]]), np.array([len(r) for r in host["rewards"]])
    print("PID, device loop against host loop: episodes with another length {}, mean |dlength| {:.3f}, settling all {:.4f} / {:.4f} s".format(
        int((lengths != lengths_host).sum()), float(np.mean(np.abs(lengths - lengths_host))), table["settling_time"]["all"],
        table_host["settling_time"]["all"]))
    for state in res["success"]:
        assert res["success"][state] == host["success"][state], state            # per scenario
    assert np.mean(np.abs(lengths - lengths_host)) < 2.0
    np.testing.assert_allclose(table["settling_time"]["all"], table_host["settling_time"]["all"], rtol=0.02)
    assert table["success_%"] == {"roll": 100.0, "pitch": 100.0, "Va": 100.0, "all": 100.0}


# ---------------------------------------------------------------------------------------------------------- PPO.evaluate
def _learner():
    from gym_fixed_wing.ppo import PPO
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    vec = FixedWingVecEnv(configs.reference_like("examples"), num_envs=256, config_kw={"steps_max": 25}, seed=3, device=0)
    vec.set_curriculum_level(0.25)
    vec.reset()
    return vec, PPO(vec, seed=0, n_steps=16, nminibatches=4, noptepochs=2, update="hip")


def test_ppo_evaluate_leaves_the_training_run_where_it_was():
    import torch
    scen = _scenarios(8)
    runs, table = [], None
    for evaluates in (False, True):
        torch.manual_seed(1234)
        vec, ppo = _learner()
        for k in range(3):
            ppo.update(ppo.collect())
            if evaluates and k == 0:
                table = ppo.evaluate(scen)
                assert set(ppo.evaluate(scen, first_step="normalised")) == set(table)
                # the evaluation head, loaded with the training head's statistics, acts as the training head does
                _, head, _ = next(iter(ppo._eval.values()))
                obs = torch.randn(8, vec.obs_dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
                twin = type(head)(8, vec.obs_dim, training=False, device=0, gamma=ppo.hp["gamma"])
                twin.load_policy(ppo.policy)
                st = ppo.actor.get_stats()
                twin.set_stats(st["obs_mean"], st["obs_var"], st["obs_count"], st["ret_mean"], st["ret_var"], st["ret_count"])
                assert torch.equal(head.act(obs, deterministic=True)[1], twin.act(obs, deterministic=True)[1])
                assert head.get_stats()["obs_mean"].tobytes() == st["obs_mean"].tobytes()
                assert head.get_stats()["obs_var"].tobytes() == st["obs_var"].tobytes()
        nxt = ppo.collect()
        runs.append({"flat": ppo.learner.flat.clone(), "exp_avg": ppo.learner.exp_avg.clone(), "stats": ppo.actor.get_stats(),
                     "actions": nxt["actions"].clone(), "gen": ppo._gen.get_state().clone(), "global": torch.rand(1)})
        vec.close()
    a, b = runs
    assert torch.equal(a["flat"], b["flat"]) and torch.equal(a["exp_avg"], b["exp_avg"])
    assert torch.equal(a["actions"], b["actions"])
    assert torch.equal(a["gen"], b["gen"]) and torch.equal(a["global"], b["global"])
    for k, v in a["stats"].items():
        assert np.asarray(v).tobytes() == np.asarray(b["stats"][k]).tobytes(), k
    want = ev.summarize({"success": {"roll": [True], "pitch": [True], "Va": [True], "all": [True]},
                         "rise_time": {"roll": [1.0], "pitch": [1.0], "Va": [1.0]}, "settling_time": {"roll": [1.0], "pitch": [1.0], "Va": [1.0], "all": [1.0]},
                         "overshoot": {"roll": [1.0], "pitch": [1.0], "Va": [1.0]}, "control_variation": {"all": [1.0]}})
    assert set(table) == set(want) and all(set(table[k]) == set(want[k]) for k in want)


def test_train_ppo_evaluates_on_the_test_set_four_times():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
    try:
        import train_ppo
    finally:
        sys.path.pop(0)
    ppo, _ = train_ppo.train(envs=256, timesteps=5 * 256 * 16, n_steps=16, nminibatches=4, noptepochs=1, log=None, update="hip",
                             test_set=_scenarios(8))
    tested = [h for h in ppo.history if "test" in h]
    assert len(ppo.history) == 5 and len(tested) == 4
    assert [h["update"] for h in tested] == [1, 2, 3, 4]
    assert all(set(h["test"]) == {"success_%", "rise_time", "settling_time", "overshoot", "control_variation"} for h in tested)
    json.dumps(ppo.history)     # what --curve writes
    ppo.vec.close()
