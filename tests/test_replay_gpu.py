"""The device hindsight replay buffer, GPU half (the CPU half and the description of the shared bodies: tests/test_replay.py,
tests/replay_common.py).

  shared       every kernel and layer test of the CPU half, on the MI355X (same inputs, same restatement, same bounds);
  device       sample() takes and returns device tensors, `out=` reused across two calls without a host copy;
  example      examples/train_her.py for two iterations in a fresh child process: exit status 0 and finite losses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import goal_common as gc
import replay_common as rc
import test_replay as cpu_half
from gym_fixed_wing.goal import GoalLog
from gym_fixed_wing.replay import HindsightReplay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kw():
    return {"device": 0}


# the bodies of the CPU half take the backend through `kw`
test_the_library_exports_the_replay_calls = cpu_half.test_the_library_exports_the_replay_calls
test_replay_index_is_the_backward_scan = cpu_half.test_replay_index_is_the_backward_scan
test_replay_sample_matches_the_restatement = cpu_half.test_replay_sample_matches_the_restatement
test_replay_sample_is_a_function_of_seed_and_serial = cpu_half.test_replay_sample_is_a_function_of_seed_and_serial
test_hindsight_replay_stores_rollouts_and_samples_them = cpu_half.test_hindsight_replay_stores_rollouts_and_samples_them
test_replay_entry_points_refuse_what_they_cannot_serve = cpu_half.test_replay_entry_points_refuse_what_they_cannot_serve


def test_sample_takes_and_returns_device_tensors_and_reuses_out(kw):
    import torch
    T, N, K, B = 8, 70, 2, 512
    vec = gc.make_env(kw, gc.goal_config("default"), N, config_kw={"steps_max": 10}, seed=2)
    replay = HindsightReplay(vec, T, K, strategy="episode", p=0.8, seed=5, target_observations="stale")
    log = GoalLog(vec, T)
    m_, D = vec._mem, vec.obs_dim
    obs = torch.zeros((T, N, D), device="cuda:0")
    acts = torch.as_tensor(np.random.default_rng(1).uniform(-1.3, 1.3, (T, N, 3)).astype(np.float32)).to("cuda:0")
    raw, dones = torch.zeros((T, N), device="cuda:0"), torch.zeros((T, N), dtype=torch.uint8, device="cuda:0")
    o = vec.reset()
    log.observe(0)
    for t in range(T):
        obs[t].copy_(torch.as_tensor(o).reshape(N, D))
        o, _, d = vec.step_device(acts[t], reward_out=raw[t])
        dones[t].copy_(d)
        log.observe(t + 1)
    replay.add(obs, torch.as_tensor(o).reshape(N, D), acts, raw, dones, log)
    out = replay.sample(B)
    for name in ("observation", "next_observation", "action", "achieved_goal", "desired_goal", "reward", "done", "index"):
        assert isinstance(out[name], torch.Tensor) and out[name].is_cuda and out[name].shape[0] == B, name
    first = {k: v.clone() for k, v in out.items()}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    again = replay.sample(B, out=out)
    assert again is out and all(out[k].data_ptr() == ptrs[k] for k in ptrs)
    assert (out["index"] != first["index"]).any() and replay.serial == 2
    # both calls against the restatement on the slot's contents
    stored = {"obs": gc.host(vec, replay.obs), "actions": gc.host(vec, replay.actions), "raw": gc.host(vec, replay.raw_rewards),
              "dones": gc.host(vec, replay.dones), "ep_end": gc.host(vec, replay.ep_end), "ach": gc.host(vec, replay.achieved),
              "des": gc.host(vec, replay.desired)}
    ref = gc.RefReward(vec)
    for call, res in enumerate((first, out)):
        got = {name: res[name].cpu().numpy() for name in ("observation", "next_observation", "action", "reward", "done", "index")}
        got["achieved"], got["desired"] = res["achieved_rows"].cpu().numpy(), res["desired_rows"].cpu().numpy()
        rc.compare(got, rc.ref_sample(ref, stored, 1, "episode", B, 5, call, replay.p_scaled), "device sample {}".format(call))
    vec.close()


def test_the_her_example_trains_for_two_iterations():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_her.py"), "--envs", "64", "--iters", "2", "--n-steps", "8", "--batch", "256"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("iter")]
    assert len(lines) == 2, r.stdout
    for l in lines:
        words = l.replace("=", " ").split()
        losses = [float(words[words.index(k) + 1]) for k in ("critic_loss", "actor_loss")]
        assert np.isfinite(losses).all(), l
