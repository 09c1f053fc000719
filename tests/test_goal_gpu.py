"""The goal-conditioned VecEnv and hindsight relabelling, GPU half (the CPU half and the description of the shared bodies:
tests/test_goal.py, tests/goal_common.py).

  shared       every kernel and layer test of the CPU half, on the MI355X (same inputs, same restatement, same bounds);
  graph replay FusedRollout(goals=log, graph=True) against an eager twin, 3 replays of 10 steps at 130 envs with steps_max 7: the goal
               rows and every rollout buffer bit-equal, and relabel on the replayed buffers against the restatement."""
import numpy as np
import pytest

import goal_common as gc
import test_goal as cpu_half
from gym_fixed_wing.goal import GoalLog
from gym_fixed_wing.rollout import FusedRollout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kw():
    return {"device": 0}


relabel_envs = cpu_half.relabel_envs

# the bodies of the CPU half take the backend through `kw`
test_the_library_exports_the_goal_calls = cpu_half.test_the_library_exports_the_goal_calls
test_goal_reward_matches_the_restatement = cpu_half.test_goal_reward_matches_the_restatement
test_goal_reward_on_the_golden_relabel_records = cpu_half.test_goal_reward_on_the_golden_relabel_records
test_goal_reward_with_a_transitions_own_goals_is_the_steps_reward = cpu_half.test_goal_reward_with_a_transitions_own_goals_is_the_steps_reward
test_goal_observe_is_the_recorders_row = cpu_half.test_goal_observe_is_the_recorders_row
test_goal_observe_without_derived_views_and_in_turbulence = cpu_half.test_goal_observe_without_derived_views_and_in_turbulence
test_goal_relabel_matches_the_restatement = cpu_half.test_goal_relabel_matches_the_restatement
test_sharded_relabels_are_the_columns_of_the_whole_and_the_serial_counts = cpu_half.test_sharded_relabels_are_the_columns_of_the_whole_and_the_serial_counts
test_entry_points_refuse_what_the_yardstick_cannot_define = cpu_half.test_entry_points_refuse_what_the_yardstick_cannot_define
test_goal_vec_env_against_the_single_env_class = cpu_half.test_goal_vec_env_against_the_single_env_class
test_goal_entries_of_matrix_observations = cpu_half.test_goal_entries_of_matrix_observations
test_rollout_with_a_goal_log_against_one_without_and_relabel = cpu_half.test_rollout_with_a_goal_log_against_one_without_and_relabel
test_rollout_refuses_a_log_without_raw_rewards_or_on_the_one_launch_step = cpu_half.test_rollout_refuses_a_log_without_raw_rewards_or_on_the_one_launch_step


def test_compute_reward_takes_and_returns_device_tensors(kw):
    import torch
    vec = gc.make_env(kw, gc.goal_config("reward_mix_potential"), 4)
    env = gc.GoalVecEnv(vec)
    ref = gc.RefReward(vec)
    ach, des, prev, win, step, _ = gc.contract_inputs(ref, 65, 1)
    win = np.nan_to_num(win)
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x)).to(device="cuda:0", dtype=dt)
    info = {"step": dev(step, torch.int32), "action_window": dev(win[:, :, :3].transpose(1, 0, 2)), "prev_state": dev(ref.unscale(prev))}
    got = env.compute_reward(dev(ach[:, :3]), dev(des[:, :3]), info)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (65,)
    want = ref(ach, des, prev, win, step, 0)
    # (prev_state travels unscaled and is scaled again in fp32: one more rounding than the contract's identical inputs)
    assert gc.rel_err(got.cpu().numpy(), want).max() <= 1e-5
    vec.close()


def test_goal_log_under_graph_replay_equals_eager():
    n, n_steps, replays = 130, 10, 3
    runs = {}
    for name, graph in (("graph", True), ("eager", False)):
        vec = gc.make_env({"device": 0}, gc.goal_config("default"), n, config_kw={"steps_max": 7}, seed=2)
        vec.reset()
        actor = gc.small_head(vec)
        log = GoalLog(vec, n_steps)
        ro = FusedRollout(vec, actor, n_steps, graph=graph, raw_rewards=True, goals=log)
        assert not ro.fused
        if not graph:                                    # the two warm-up steps a capture takes before it records the graph
            ro._prime()
            ro._step(ro.cur["actions"], ro.cur)
            ro._step(ro.cur["actions"], ro.cur)
        runs[name] = (vec, actor, ro, log)
    vec, _, ro, log = runs["graph"]
    ref = gc.RefReward(vec)
    dones = 0
    for r in range(replays):
        bufs = {name: {k: v.cpu().numpy() for k, v in ro_.run().items()} for name, (_, _, ro_, _) in runs.items()}
        rows = {name: (log_.achieved.cpu().numpy(), log_.desired.cpu().numpy()) for name, (_, _, _, log_) in runs.items()}
        for k in bufs["eager"]:
            np.testing.assert_array_equal(bufs["graph"][k].view(np.uint8), bufs["eager"][k].view(np.uint8), err_msg="replay {} buffer {}".format(r, k))
        for i, what in enumerate(("achieved", "desired")):
            np.testing.assert_array_equal(rows["graph"][i].view(np.int32), rows["eager"][i].view(np.int32), err_msg="replay {}: {} rows".format(r, what))
        ach, des = rows["graph"]
        idx = ach[:, :, 3].view(np.uint32) & 0xFFFF
        d = bufs["graph"]["dones"] != 0
        assert (idx[1:][d] == 0).all() and (idx[1:][~d] == idx[:-1][~d] + 1).all() and ach[:, :, :3].any()
        dones += int(d.sum())
        out = log.relabel(ro.buf, p=0.8, seed=3)
        src, rew = out["src_row"].cpu().numpy(), out["rewards"].cpu().numpy()
        w_src, w_des, w_rew, rel = gc.ref_relabel(ref, ach, des, bufs["graph"]["actions"], bufs["graph"]["raw_rewards"], bufs["graph"]["dones"], 3, r,
                                                  min(1 << 32, int(round(0.8 * 2.0 ** 32))))
        np.testing.assert_array_equal(src, w_src)
        np.testing.assert_array_equal(out["desired_goal"].cpu().numpy().view(np.int32), w_des.view(np.int32))
        np.testing.assert_array_equal(rew[~rel].view(np.int32), bufs["graph"]["raw_rewards"][~rel].view(np.int32))
        assert rel.any() and gc.rel_err(rew[rel], w_rew[rel]).max() <= gc.REWARD_TOL
    assert dones >= n * (replays * n_steps // 7 - 1)
    for v, actor, _, _ in runs.values():
        actor.close()
        v.close()
