"""The goal-conditioned VecEnv and hindsight relabelling (include/fwgym.h "Goal env", gym_fixed_wing.goal) on the HOST EMULATION of
the kernels -- the CPU half; tests/test_goal_gpu.py is the GPU half and shares the bodies (tests/goal_common.py).

  yardstick  the numpy restatement of the reward against FixedWingAircraftGoal.compute_reward over the golden 14-step episode and
             against the recorded reference rewards of tests/golden/g4_goal_*.json;
  reward     fwg_goal_reward against the restatement on identical fp32 inputs: four configurations, m = 1 / 63 / 64 / 65 / 257, steps
             0 / 1 / 2 / W - 1 / W / 500, roll errors across +-pi, NaN window rows, guard rows; the golden records; the anchor to the
             step kernel's reward (mode 1 equal, mode 0 off at transition 1 only);
  observe    fwg_goal_observe bit-equal to a FlightRecorder's rows, N = 1 / 63 / 64 / 130, derived views on / off, turbulence;
  relabel    fwg_goal_relabel against the restatement on synthetic rollouts (T x N grid, every done pattern, p = 0 / 2^31 / 2^32),
             the generator itself, sharding, the serial;
  refusals   status codes and messages, nothing launched;
  layers     GoalVecEnv against the single-env class, matrix observations, FusedRollout(goals=log) against a twin, relabel on a
             real rollout, the kernels' resources."""
import os

import numpy as np
import pytest

import goal_common as gc
from emu.host_backend import HERE as EMU_HERE, HostBackend, build_emu as _build_emu
from gym_fixed_wing import _native as nat

# tools/mutation_check.py re-runs this file against kernel sources with a bug put in (the goal_* mutants)
MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")


def build_emu():
    return _build_emu(src=MUT_SRC, out=os.path.join(EMU_HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else _build_emu()


@pytest.fixture(scope="module")
def kw():
    return {"_backend": HostBackend(), "_lib_path": build_emu()}


@pytest.fixture(scope="module")
def relabel_envs(kw):
    """One env per N of the relabel grid (the calls need a handle of N envs), reward_mix in the potential form: every factor class."""
    envs = {}

    def get(n):
        if n not in envs:
            vec = gc.make_env(kw, gc.goal_config("reward_mix_potential"), n)
            envs[n] = (vec, gc.RefReward(vec))
        return envs[n]
    yield get
    for vec, _ in envs.values():
        vec.close()


def test_the_library_exports_the_goal_calls(kw):
    lib = nat.load_library(kw.get("_lib_path"))
    assert {"fwg_goal_window", "fwg_goal_observe", "fwg_goal_reward", "fwg_goal_relabel"} <= set(nat.PROTOTYPES)
    assert all(hasattr(lib, n) for n in nat.PROTOTYPES if n.startswith("fwg_goal_"))
    assert nat.STREAM_GOAL == 10 and (nat.GOAL_KEPT, nat.GOAL_TERMINAL, nat.GOAL_NO_WINDOW) == (-1, -2, -3)
    vec = gc.make_env(kw, gc.goal_config("default"), 1)
    assert gc.gl.goal_window(vec) == 5
    vec.close()


# -------------------------------------------------------------------------------------------------------- 1. yardstick first
@pytest.mark.parametrize("form", ["absolute", "potential"])
def test_the_restatement_is_the_single_env_compute_reward(kw, form):
    print("restatement vs compute_reward, {}: {:.3g}".format(form, gc.yardstick_episode(kw, form)))
    print("restatement vs recorded reference rewards, {}: {:.3g}".format(form, gc.yardstick_golden(kw, form)))


# ------------------------------------------------------------------------------------------------------------- 2. the reward
@pytest.mark.parametrize("m", gc.CONTRACT_M)
@pytest.mark.parametrize("kind", gc.KINDS)
def test_goal_reward_matches_the_restatement(kw, kind, m):
    worst = gc.reward_contract(kw, kind, m)
    print("fwg_goal_reward {} m {}: worst relative error {:.3g}".format(kind, m, worst))
    assert worst <= gc.REWARD_TOL <= 1e-5, worst


def test_the_contract_inputs_hold_the_cases_that_matter(kw):
    vec = gc.make_env(kw, gc.goal_config("reward_mix_potential"), 1)
    ref = gc.RefReward(vec)
    ach, des, prev, win, step, _ = gc.contract_inputs(ref, 257, 0)
    W = ref.window
    assert W == 5 and set(step) == {0, 1, 2, W - 1, W, 500}
    raw = ref.unscale(ach)[:, 0] - ref.unscale(des)[:, 0]
    assert (raw > np.pi).any() and (raw < -np.pi).any() and (np.abs(raw) < 0.05).any()
    err = ref.errors(ref.unscale(ach), ref.unscale(des))
    for n, b in ref.bounds.items():
        assert np.abs(np.abs(err[n]) - b).min() >= 2e-4 and (np.abs(err[n]) <= b).any() and (np.abs(err[n]) > b).any(), n
    assert np.isnan(win[W - 2, step == 0]).all() and not np.isnan(win[W - 1]).any() and not np.isnan(win[:, step >= W - 1]).any()
    assert (np.abs(win[W - 1, :, :3]) > 1.5).any()
    vec.close()


@pytest.mark.parametrize("form", ["absolute", "potential"])
def test_goal_reward_on_the_golden_relabel_records(kw, form):
    worst = gc.reward_golden(kw, form)
    print("fwg_goal_reward vs recorded reference rewards, {}: {:.3g}".format(form, worst))
    assert worst <= gc.GOLDEN_TOL <= 2e-4, worst


@pytest.mark.parametrize("form", ["absolute", "potential"])
def test_goal_reward_with_a_transitions_own_goals_is_the_steps_reward(kw, form):
    worst = gc.anchor_to_the_step(kw, form)
    print("fwg_goal_reward mode 1 vs the step's reward, {}: {:.3g}".format(form, worst))
    assert worst <= gc.ANCHOR_TOL <= 5e-5, worst


# ------------------------------------------------------------------------------------------------------------ 3. the observe
@pytest.mark.parametrize("n", [1, 63, 64, 130])
def test_goal_observe_is_the_recorders_row(kw, n):
    gc.observe_against_the_recorder(kw, n)


def test_goal_observe_without_derived_views_and_in_turbulence(kw):
    gc.observe_against_the_recorder(kw, 63, derived_views=False)
    gc.observe_against_the_recorder(kw, 63, derived_views=False, turbulence=True)
    gc.observe_against_the_recorder(kw, 63, derived_views=True, turbulence=True)


# ------------------------------------------------------------------------------------------------------------ 4. the relabel
def test_the_synthetic_rollouts_hold_the_cases_that_matter(relabel_envs):
    """Pure numpy: the generator and the restatement on the [300][130] case."""
    _, ref = relabel_envs(1)
    T, N = 300, 130
    ach, des, actions, raw, dones = gc.synthetic(ref, T, N)
    for name, d in gc.grid_clearance(ref.bounds).items():
        assert d > 2e-4, (name, d)
    assert not dones[:, 0].any() and dones[:, 1].all() and dones[:, 2].sum() == 1 == dones[0, 2] and dones[:, 3].sum() == 1 == dones[T - 1, 3]
    assert list(np.flatnonzero(dones[:, 7])) == [0, 127, 128, 255, 256]
    src, _, _, rel = gc.ref_relabel(ref, ach, des, actions, raw, dones, 1, 0, 1 << 32)
    counts = {k: int((src == k).sum()) for k in (-1, -2, -3)}
    assert counts[-1] == 0 and counts[-2] >= 100 and counts[-3] >= 100 and rel.sum() >= 100
    assert rel.sum() > max(counts.values())                                # relabelled is the most frequent outcome
    tt, nn = np.nonzero(rel)
    nxt = np.array([[min([t2 for t2 in range(t + 1, T) if dones[t2, n]] + [T]) for n in range(N)] for t in range(T)])
    assert (src[tt, nn] == tt + 1).any() and (src[tt, nn] == nxt[tt, nn]).any() and (nxt[tt, nn] == T).any()
    assert (src[tt, nn] > tt).all() and (src[tt, nn] <= nxt[tt, nn]).all()
    half, _, _, _ = gc.ref_relabel(ref, ach, des, actions, raw, dones, 1, 0, 1 << 31)
    drawn = (half == -1) | (half >= 0)
    assert 0.4 < (half == -1).sum() / drawn.sum() < 0.6
    none, _, _, _ = gc.ref_relabel(ref, ach, des, actions, raw, dones, 1, 0, 0)
    assert not (none >= 0).any()


@pytest.mark.parametrize("t", gc.RELABEL_T)
@pytest.mark.parametrize("n", gc.RELABEL_N)
def test_goal_relabel_matches_the_restatement(relabel_envs, n, t):
    vec, ref = relabel_envs(n)
    out = gc.relabel_cell(vec, ref, t)
    assert not (out[0] >= 0).any()


def test_sharded_relabels_are_the_columns_of_the_whole_and_the_serial_counts(kw):
    gc.sharding_case(kw)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_entry_points_refuse_what_the_yardstick_cannot_define(kw):
    res = gc.refusals(kw)
    assert len(res) == 20, sorted(res)
    assert "reward factor" in res["int_error"] and "int_error" in res["int_error"]
    assert "slot 2" in res["error factor of a non-goal"] or "target slot 2" in res["error factor of a non-goal"]


# ------------------------------------------------------------------------------------------------------ 6. through the layers
@pytest.mark.parametrize("form", ["absolute", "potential"])
def test_goal_vec_env_against_the_single_env_class(kw, form):
    gc.goal_vec_env_against_the_single_env(kw, form)


def test_goal_entries_of_matrix_observations(kw):
    gc.matrix_observation_goals(kw)


def test_rollout_with_a_goal_log_against_one_without_and_relabel(kw):
    gc.rollout_with_and_without_the_log(kw)


def test_rollout_refuses_a_log_without_raw_rewards_or_on_the_one_launch_step(kw):
    gc.rollout_refusals(kw)


def test_goal_kernels_use_no_scratch_and_spill_nothing():
    """The committed resource report of the product build (gym_fixed_wing/kernel_resources.json, whose source hash
    tests/test_kernel_resources.py pins) lists the goal kernels: no scratch frame, no spills."""
    import json
    from gym_fixed_wing import specialize
    with open(specialize.RESOURCES_JSON) as f:
        kernels = json.load(f)["kernels"]
    found = {n.split("(")[0]: r for n, r in kernels.items() if n.startswith("k_goal")}
    assert set(found) == {"k_goal_observe", "k_goal_reward", "k_goal_relabel", "k_goal_relabel_reward"}, sorted(found)
    for name, r in found.items():
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            assert r[key] == 0, (name, key, r[key])
