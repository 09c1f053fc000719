"""The device training monitor (include/fwgym.h "Training monitor", gym_fixed_wing.monitor) on the HOST EMULATION of the kernels
-- the CPU half; tests/test_monitor_gpu.py is the GPU half and shares the bodies (tests/monitor_common.py).

  contract   fwg_monitor_fold / fwg_monitor_take against the numpy restatement on synthetic rollouts, all 8 outputs and both
             carries bit for bit: env counts 1 / 63 / 64 / 130 / 4096, rollouts of 1 / 7 / 127 / 128 / 129 / 300 steps (the
             kernel's span is 128, its segments 32), every done pattern per env (never, every step, first, last, on both sides of
             every segment boundary, Bernoulli), rewards of both signs with exact ties, the bound itself, NaN / inf / 2e6;
  carry      an episode through three folds, two folds before one take, a take of nothing, a second take;
  sharding   the fold of [T][130] equals the combination of the folds of its columns [0, 37) and [37, 130);
  refusals   status codes, nothing launched;
  layers     FusedRollout(raw_rewards=True) against a tap and a twin, the recorder beside the monitor, PPO(monitor=True) against
             PPO(monitor=False), window(), vec.reset(), ProgressLog, two gloo ranks."""
import os
import sys

import numpy as np
import pytest

import monitor_common as mc
from emu.host_backend import HERE as EMU_HERE, HostBackend, build_emu as _build_emu
from gym_fixed_wing import _native as nat
from gym_fixed_wing import monitor as mon

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# tools/mutation_check.py re-runs this file against kernel sources with a bug put in (the monitor_* mutants)
MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")


def build_emu():
    return _build_emu(src=MUT_SRC, out=os.path.join(EMU_HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else _build_emu()


@pytest.fixture(scope="module")
def kw():
    return {"_backend": HostBackend(), "_lib_path": build_emu()}


# ------------------------------------------------------------------------------------------------------------ 1. contract
def test_abi_26_exports_the_monitor(kw):
    lib = nat.load_library(kw.get("_lib_path"))
    assert nat.FWG_ABI_VERSION == 26 == lib.fwg_abi_version() and nat.N_MONITOR == 8
    assert {"fwg_monitor_scratch_bytes", "fwg_monitor_fold", "fwg_monitor_take"} <= set(nat.PROTOTYPES)


@pytest.mark.parametrize("t", mc.CONTRACT_T)
@pytest.mark.parametrize("n", mc.CONTRACT_N)
def test_fold_and_take_match_the_numpy_restatement_bit_for_bit(kw, n, t):
    mc.run_contract(kw, n, t)


def test_synthetic_rollouts_hold_the_cases_that_matter():
    rew, done = mc.synthetic(300, 130)
    assert len(mc.PATTERNS) == 9 and not done[:, 0].any() and done[:, 1].all()
    assert done[:, 2].sum() == 1 == done[0, 2] and done[:, 3].sum() == 1 == done[299, 3]
    assert list(np.flatnonzero(done[:, 4])) == [31, 63, 95, 127, 159, 191, 223, 255, 287]       # s0 - 1 / s1 - 1
    assert list(np.flatnonzero(done[:, 5])) == [0, 32, 64, 96, 128, 160, 192, 224, 256, 288]    # s0
    q = rew.astype(np.float64) * 2 ** 20
    ok = np.abs(rew) <= mc.SCALE
    assert (rew[ok] < 0).any() and (rew[ok] > 0).any() and (np.abs(q[ok] - np.floor(q[ok])) == 0.5).sum() > 1000
    assert np.isnan(rew).any() and np.isinf(rew).any() and (rew == np.float32(2e6)).any() and (np.abs(rew) == mc.SCALE).any()


def test_a_bad_reward_flags_exactly_one_episode(kw):
    """Per value (NaN, inf, 2e6): before or on the first done flags the first episode, after it the second; the other episode
    of the env counts, with the good rewards only."""
    got = mc.bad_reward_cases(kw)
    assert got[1] == 9 and got[0] == 9                           # 18 episodes, one flagged per env
    assert got[6] == 4 and got[7] == 5 and got[4] == 4 * 0.25 and got[5] == 5 * 0.25


def test_carries_and_takes(kw):
    out = mc.carry_cases(kw)
    inf = float("inf")
    for name in ("empty", "again"):
        assert list(out[name]) == [0, 0, 0, 0, inf, -inf, inf, -inf], name
    assert out["two_folds"][0] > 50


def test_sharded_folds_combine_to_the_whole(kw):
    mc.sharding_case(kw)


def test_entry_points_refuse_bad_arguments(kw):
    res = mc.refusals(kw)
    assert len(res) == 12
    for name, (status, msg) in res.items():
        assert status == -1, name                                # FWG_ERR_INVALID
        assert msg.startswith("fwg_monitor_take" if name.startswith("take") else "fwg_monitor_fold"), (name, msg)


def test_monitor_kernels_use_no_scratch_and_spill_nothing():
    """The committed resource report of the product build (gym_fixed_wing/kernel_resources.json, whose source hash
    tests/test_kernel_resources.py pins) lists the two monitor kernels: no scratch frame, no spills."""
    import json
    from gym_fixed_wing import specialize
    with open(specialize.RESOURCES_JSON) as f:
        kernels = json.load(f)["kernels"]
    found = {n.split("(")[0]: r for n, r in kernels.items() if n.startswith("k_monitor")}
    assert set(found) == {"k_monitor_fold", "k_monitor_take"}, sorted(found)
    for name, r in found.items():
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            assert r[key] == 0, (name, key, r[key])


# ---------------------------------------------------------------------------------------------------- 2. through the layers
def test_raw_rewards_rollout_against_the_tap_and_a_twin(kw):
    mc.raw_rewards_rollout(kw)


def test_the_one_launch_step_refuses_raw_rewards(kw):
    mc.one_launch_step_refuses_raw_rewards(kw)


def test_recorder_and_monitor_together(kw):
    mc.recorder_and_monitor_together(kw)


def test_window_pools_several_takes_at_4_envs(kw):
    mc.window_pools_takes(kw)


def test_reset_zeroes_the_carries(kw):
    mc.reset_zeroes_the_carries(kw)


def test_ppo_with_and_without_the_monitor_and_the_progress_log(kw, tmp_path):
    mc.ppo_with_and_without_the_monitor(kw, str(tmp_path / "log"))


def test_progress_log_keeps_the_first_rows_keys(tmp_path):
    lines = []
    log = mon.ProgressLog(str(tmp_path), log_interval=2, out=lines.append)
    ep = {"episodes": 3, "success": {"roll": 0.5, "all": 0.25}, "control_variation": {"all": 1.0}}
    log({"update": 1, "ep_rew_mean": None, "ep_info": ep, "curve": [1, 2]})
    log({"update": 2, "ep_rew_mean": -1.5, "extra": 7, "ep_info": dict(ep, episodes=0)})
    log({"update": 3})
    log({"update": 4, "ep_rew_mean": 2.0, "ep_info": ep})
    with open(log.path) as f:
        text = f.read().splitlines()
    assert text[0] == "update,ep_rew_mean,ep_info/episodes,ep_info/success/roll,ep_info/success/all,ep_info/control_variation/all"
    assert text[1:] == ["1,,3,0.5,0.25,1.0", "2,-1.5,0,0.5,0.25,1.0", "3,,,,,", "4,2.0,3,0.5,0.25,1.0"]
    assert lines == ["\nsuccess:\n\troll      0.50\n\tall       0.25\ncontrol_variation:\n\tall       1.00"]   # (call 2 had no episode)


# ------------------------------------------------------------------------------------------------------------ 3. two ranks
TOTAL, T_RANKS = 130, 140


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import json
    import monitor_common as mc_
    from gym_fixed_wing import distributed as fd
    first, n = fd.shard(TOTAL, rank, world)
    rew, done = mc_.synthetic(T_RANKS, TOTAL, seed=9)
    m = mc_.bare_monitor({"_backend": HostBackend(), "_lib_path": build_emu()}, n)
    mc_.fold(m, np.ascontiguousarray(rew[:, first:first + n]), np.ascontiguousarray(done[:, first:first + n]))
    with open(os.path.join(out_dir, "take_{}.json".format(rank)), "w") as f:
        json.dump([m.take(), m.window(100), m.take()], f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_report_the_one_rank_take(kw, tmp_path):
    import json
    import torch.multiprocessing as mp
    build_emu()
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (json.load(open(tmp_path / "take_{}.json".format(r))) for r in range(2))
    rew, done = mc.synthetic(T_RANKS, TOTAL, seed=9)
    one = mc.bare_monitor(kw, TOTAL)
    mc.fold(one, rew, done)
    want = one.take()
    assert a == b and a[0] == want and want["episodes"] > 100 and want["nonfinite"] > 0
    assert a[1] == one.window(100) and a[2]["episodes"] == 0 and a[2]["ep_rew_mean"] is None
