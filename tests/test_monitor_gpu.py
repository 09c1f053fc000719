"""The device training monitor, GPU half (the CPU half and the description of the shared bodies: tests/test_monitor.py,
tests/monitor_common.py).

  shared       every kernel and layer test of the CPU half, on the MI355X (same inputs, same restatement, bit for bit);
  graph replay FusedRollout(raw_rewards=True) captured into a hipGraph against an eager twin and against a captured rollout without
               the flag, 12 replays at 4 096 envs x 8 steps with steps_max 20, dense observations with an attached MLP head and the
               row log with the CNN head: every buffer bit-equal (the launch counts are compared by the shared eager test), and after
               every replay the monitor's take equals the numpy fold of the buffers read back."""
import numpy as np
import pytest
import torch

import configs
import monitor_common as mc
import test_monitor as cpu_half
from gym_fixed_wing.actor import DeviceActor
from gym_fixed_wing.monitor import EpisodeMonitor
from gym_fixed_wing.rollout import CnnMlpPolicy, FusedRollout, MlpPolicy
from gym_fixed_wing.vec_env import FixedWingVecEnv

pytestmark = pytest.mark.gpu
GRAPH_N, GRAPH_STEPS_MAX = 4096, 20


@pytest.fixture(scope="module")
def kw():
    return {"device": 0}


# the bodies of the CPU half take the backend through `kw`
test_abi_26_exports_the_monitor = cpu_half.test_abi_26_exports_the_monitor
test_fold_and_take_match_the_numpy_restatement_bit_for_bit = cpu_half.test_fold_and_take_match_the_numpy_restatement_bit_for_bit
test_a_bad_reward_flags_exactly_one_episode = cpu_half.test_a_bad_reward_flags_exactly_one_episode
test_carries_and_takes = cpu_half.test_carries_and_takes
test_sharded_folds_combine_to_the_whole = cpu_half.test_sharded_folds_combine_to_the_whole
test_entry_points_refuse_bad_arguments = cpu_half.test_entry_points_refuse_bad_arguments
test_raw_rewards_rollout_against_the_tap_and_a_twin = cpu_half.test_raw_rewards_rollout_against_the_tap_and_a_twin
test_the_one_launch_step_refuses_raw_rewards = cpu_half.test_the_one_launch_step_refuses_raw_rewards
test_recorder_and_monitor_together = cpu_half.test_recorder_and_monitor_together
test_window_pools_several_takes_at_4_envs = cpu_half.test_window_pools_several_takes_at_4_envs
test_reset_zeroes_the_carries = cpu_half.test_reset_zeroes_the_carries
test_ppo_with_and_without_the_monitor_and_the_progress_log = cpu_half.test_ppo_with_and_without_the_monitor_and_the_progress_log


# ---------------------------------------------------------------------------------------------------------- under graph replay
def _env(preset):
    return FixedWingVecEnv(configs.reference_like(preset), num_envs=GRAPH_N, device=0, config_kw={"steps_max": GRAPH_STEPS_MAX},
                           derived_views=preset == "cnn", seed=2)


def _head(vec, preset):
    torch.manual_seed(0)
    policy = CnnMlpPolicy(obs_shape=vec.obs_shape, n_filters=3) if preset == "cnn" else MlpPolicy(vec.obs_dim)
    with torch.no_grad():
        policy.log_std.copy_(torch.tensor([-1.0, -0.7, -1.2]))
        if preset == "cnn":
            policy.conv.weight.normal_(0.0, 0.5)
    actor = DeviceActor.for_env(vec, seed=5)
    actor.load_policy(policy.cuda() if preset == "cnn" else policy)
    return actor


@pytest.mark.parametrize("preset", ["examples", "cnn"])
def test_raw_rewards_under_graph_replay_equal_eager_and_perturb_nothing(preset):
    n_steps, replays = 8, 12
    runs = {}
    for name, graph, raw in (("graph", True, True), ("eager", False, True), ("plain", True, False)):
        vec = _env(preset)
        assert bool(vec.obs_log_rows) == (preset == "cnn")
        vec.reset()
        actor = _head(vec, preset)
        ro = FusedRollout(vec, actor, n_steps, graph=graph, raw_rewards=raw)
        assert not ro.fused
        if not graph:                                    # the two warm-up steps a capture takes before it records the graph
            ro._prime()
            ro._step(ro.cur["actions"], ro.cur)
            ro._step(ro.cur["actions"], ro.cur)
        runs[name] = (vec, actor, ro)
    vec, _, ro = runs["graph"]
    assert ro.warmup is not None and runs["plain"][2].warmup is None and runs["eager"][2].warmup is None
    m, ref = EpisodeMonitor(vec), mc.RefMonitor(GRAPH_N)
    m.fold(*ro.warmup)                                   # the capture's two env steps belong to the episodes too
    ref.fold(ro.warmup[0].cpu().numpy(), ro.warmup[1].cpu().numpy())
    episodes = []
    for r in range(replays):
        bufs = {name: {k: v.cpu().numpy() for k, v in ro_.run().items()} for name, (_, _, ro_) in runs.items()}
        raw = bufs["graph"].pop("raw_rewards")
        np.testing.assert_array_equal(raw.view(np.int32), bufs["eager"].pop("raw_rewards").view(np.int32), err_msg="rollout {}: raw rewards".format(r))
        for k in bufs["plain"]:
            np.testing.assert_array_equal(bufs["graph"][k].view(np.uint8), bufs["plain"][k].view(np.uint8),
                                          err_msg="rollout {} buffer {}: raw_rewards on vs off".format(r, k))
            np.testing.assert_array_equal(bufs["graph"][k].view(np.uint8), bufs["eager"][k].view(np.uint8),
                                          err_msg="rollout {} buffer {}: graph vs eager".format(r, k))
        m.fold(ro.buf["raw_rewards"], ro.buf["dones"])
        ref.fold(raw, bufs["graph"]["dones"])
        episodes.append(int(mc.assert_same(m, ref, "replay {}".format(r))[0]))
    assert sum(episodes[:3]) > 0 and sum(episodes) >= GRAPH_N * ((2 + n_steps * replays) // GRAPH_STEPS_MAX - 1)
    for v, actor, _ in runs.values():
        actor.close()
        v.close()


def test_train_ppo_logs_the_monitor_and_checkpoints(tmp_path):
    """examples/train_ppo.py's train(monitor=True, log_dir=..., checkpoint_every=...): progress.csv has one row per update with the
    monitor's columns, the checkpoint is written, and the per-update line carries ep_rew / ep_len once episodes have ended."""
    import csv
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_ppo
    lines = []
    ck = str(tmp_path / "model.npz")
    ppo, res = train_ppo.train(envs=256, timesteps=4 * 256 * 16, n_steps=16, nminibatches=4, noptepochs=1, log=lines.append, monitor=True,
                               log_dir=str(tmp_path / "log"), log_interval=1, checkpoint_every=0.0, checkpoint_path=ck)
    assert ppo.monitor is not None and "raw_rewards" in ppo.rollout.buf and res["checkpoints"] == 4 and os.path.exists(ck)
    with open(res["progress"], newline="") as f:
        rows = list(csv.reader(f))
    assert len(rows) == 5 and {"ep_rew_mean", "ep_len_mean", "monitor_episodes", "nonfinite", "ep_rew_mean_100"} <= set(rows[0])
    assert [int(r[rows[0].index("update")]) for r in rows[1:]] == [1, 2, 3, 4]
    for info in ppo.history:
        assert info["nonfinite"] == 0 and (info["ep_rew_mean"] is None) == (info["monitor_episodes"] == 0)
    shown = [l for l in lines if "ep_rew" in l]
    assert len(shown) == sum(1 for i in ppo.history if i["monitor_episodes"] > 0 and i["episodes"] > 0)
    ppo.actor.close()
    ppo.vec.close()
