"""The device flight recorder (include/fwgym.h "Flight recorder", gym_fixed_wing.recorder) on the HOST EMULATION of the kernels
-- the CPU half; tests/test_recorder_gpu.py is the GPU half and shares the bodies (tests/recorder_common.py).

  contract   fwg_record_start / fwg_record against a thirty-line numpy restatement on scripted inputs, bit for bit: wave tails,
             ids first / last / repeated / outside the batch, 64 tracked envs, auto-reset on and off, an env done at step 0 and on
             consecutive steps, NaN rewards, a masked start in the middle, overflow (max_rows 5), sentinels behind every buffer;
  facade     Episode.states / .history of a recorded env equal the single-env class's histories exactly (auto-reset off),
             through a mid-episode reset and through an episode that ends in a constraint violation;
  auto-reset against a stepping loop with host reads, all three termination kinds;
  derived    store_derived off: the computed words against float64, calm and in turbulence;
  host       render / save_history / env_method, refusals, detach."""
import copy
import os

import numpy as np
import pytest

import configs
import recorder_common as rc
from emu.host_backend import HERE as EMU_HERE, HostBackend, build_emu as _build_emu
from gym_fixed_wing import _native as nat
from gym_fixed_wing.recorder import FlightRecorder
from gym_fixed_wing.vec_env import FixedWingVecEnv

# tools/mutation_check.py re-runs this file against kernel sources with a bug put in (the recorder_* mutants)
MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")
# Twice the worst scaled error of the computed words 16..21 against float64 (profiles/recorder_errors.txt: emulation and MI355X)
DERIVED_BOUND = 2.0 * rc.DERIVED_WORST


def build_emu():
    return _build_emu(src=MUT_SRC, out=os.path.join(EMU_HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else _build_emu()


@pytest.fixture(scope="module")
def kw():
    return {"_backend": HostBackend(), "_lib_path": build_emu()}


# ------------------------------------------------------------------------------------------------------------ 1. contract
@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("n", rc.CONTRACT_N)
def test_kernels_match_the_numpy_restatement_bit_for_bit(kw, n, auto_reset):
    for name, ids in rc.contract_id_sets(n).items():
        for max_rows in (rc.CONTRACT_T + 2, 5):          # every row fits / overflow
            rc.assert_contract(*rc.run_contract(kw, n, auto_reset, max_rows, ids))


def test_contract_script_holds_the_cases_that_matter(kw):
    """The scripted run itself: episodes that end at step 0 and on consecutive steps, envs that never end, an overflow, a slot
    whose id lies outside the batch, and a masked start that leaves the unselected envs' slabs and headers alone."""
    out = rc.run_contract(kw, 65, True, 5, list(range(10)) + [65])
    rc.assert_contract(*out)
    w_rows, w_hdr = out[2], out[3]
    assert (w_hdr[:10, 6] >= 2).sum() >= 4 and (w_hdr[1, 6] == 0)                       # e % 5 == 1 never ends
    assert (w_hdr[:, 0] & nat.REC_OVERFLOW).any() and (w_hdr[:, 0] & nat.REC_OVERFLOW_DONE).any()
    assert w_hdr[10, 0] == nat.REC_INVALID and (w_hdr[10, 1:] == 0).all()
    assert np.isnan(w_rows[..., 28]).any() and np.isnan(w_rows[..., 0]).any()
    # the masked start (even envs) re-opened env 0's episode and left env 1's alone: env 1 never ends, so its open slab holds
    # every step of the run up to the overflow
    out = rc.run_contract(kw, 65, False, rc.CONTRACT_T + 2, [0, 1])
    rc.assert_contract(*out)
    w_off = out[3]
    assert w_off[1, 1] == rc.CONTRACT_T + 1 and w_off[0, 1] < rc.CONTRACT_T + 1


def test_entry_points_refuse_bad_arguments(kw):
    for name, (status, msg) in rc.record_refusals(kw).items():
        assert status == -1, name                                        # FWG_ERR_INVALID
        assert msg.startswith("fwg_record"), (name, msg)


def test_recorder_kernels_use_no_scratch_and_spill_nothing():
    """The committed resource report of the product build (gym_fixed_wing/kernel_resources.json, whose source hash
    tests/test_kernel_resources.py pins) lists the two recorder kernels: no scratch frame, no spills, no LDS."""
    import json
    from gym_fixed_wing import specialize
    with open(specialize.RESOURCES_JSON) as f:
        kernels = json.load(f)["kernels"]
    found = {n.split("(")[0]: r for n, r in kernels.items() if n.startswith("k_record")}
    assert set(found) == {"k_record", "k_record_start"}, sorted(found)
    for name, r in found.items():
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]"):
            assert r[key] == 0, (name, key, r[key])


# ---------------------------------------------------------------------------------------------- 2. against the single-env class
def _examples(steps_max=40, **more):
    return configs.reference_like("examples"), dict({"steps_max": steps_max}, **more)


def test_recorded_episode_equals_the_single_env_history(kw, tmp_path):
    cfg, ckw = _examples()
    rng = np.random.default_rng(0)
    actions, others = rc._f32_actions(rng, 45, 1.0), rng.uniform(-1, 1, size=(45, 5, 3)).astype(np.float32)
    env, states, hist, termination, steps = rc.facade_episode(kw, cfg, ckw, actions)
    assert steps == 40 and termination == "steps"
    vec, rec = rc.vec_with_recorder(kw, cfg, ckw, auto_reset=False)
    vec.reset()
    rc.reset_env(vec, 3)
    assert rc.run_vec_episode(vec, 3, actions, others) == (40, "steps")
    for t in range(40, 45):                                    # a finished env keeps reporting done: only the first end counts
        a = others[t].copy()
        a[3] = actions[t]
        vec.step(a)
    assert rec.completed(0) == 1
    ep = rec.episode(0, "last")
    rc.assert_same_history(ep, states, hist, termination, steps)
    assert len(ep.states["roll"]) == 41 and len(ep.states["elevator"]["command"]) == 40     # the terminal state is there
    # save_history writes the single-env class's dict
    names = ["roll", "pitch", "Va", "elevator"]
    env.save_history(str(tmp_path / "facade.npy"), names)
    rec.save_history(str(tmp_path / "recorder.npy"), names)
    a, b = (np.load(str(tmp_path / f), allow_pickle=True).item() for f in ("facade.npy", "recorder.npy"))
    assert a == b and set(a) == {"roll", "pitch", "Va", "elevator", "roll_target", "pitch_target", "Va_target"}
    env.close(), vec.close()


def test_an_abandoned_episode_is_never_completed(kw):
    cfg, ckw = _examples()
    rng = np.random.default_rng(1)
    actions, others = rc._f32_actions(rng, 60, 1.0), rng.uniform(-1, 1, size=(60, 5, 3)).astype(np.float32)
    env, states, hist, termination, steps = rc.facade_episode(kw, cfg, ckw, actions[15:])
    vec, rec = rc.vec_with_recorder(kw, cfg, ckw, auto_reset=False)
    vec.reset()
    for t in range(15):
        vec.step(others[t])
    assert rec.episode(0, "current").length == 15 and rec.completed(0) == 0
    rc.reset_env(vec, 3)                                         # mid-episode: the 15 steps are dropped
    assert rec.episode(0, "current").length == 0 and rec.completed(0) == 0
    assert rc.run_vec_episode(vec, 3, actions[15:], others[15:]) == (steps, termination)
    assert rec.completed(0) == 1
    rc.assert_same_history(rec.episode(0, "last"), states, hist, termination, steps)
    env.close(), vec.close()


def test_a_failed_episode_has_no_terminal_state_row_as_in_the_single_env_class(kw):
    cfg = configs.reference_like("integrator")
    ckw = dict({"steps_max": 30}, **copy.deepcopy(rc.FAIL_PRONE))
    rng = np.random.default_rng(5)
    state = dict(rc.STATE, roll=0.5)
    for attempt in range(4):
        actions, others = rc._f32_actions(rng, 30, 1.8), rng.uniform(-1, 1, size=(30, 5, 3)).astype(np.float32)
        env, states, hist, termination, steps = rc.facade_episode(kw, cfg, ckw, actions, state=state)
        if termination not in ("steps", "success"):
            break
        env.close()
    assert termination not in ("steps", "success"), "none of the scripted episodes ended in a constraint violation"
    vec, rec = rc.vec_with_recorder(kw, cfg, ckw, auto_reset=False)
    vec.reset()
    rc.reset_env(vec, 3, state=state)
    assert rc.run_vec_episode(vec, 3, actions, others) == (steps, termination)
    ep = rec.episode(0, "last")
    rc.assert_same_history(ep, states, hist, termination, steps)
    assert len(ep.states["roll"]) == steps and len(ep.history["action"]) == steps and len(ep.history["reward"]) == steps - 1
    assert np.isnan(ep.rows[-1, :25]).all() and not np.isnan(ep.rows[-1, 25:29]).any()
    env.close(), vec.close()


# ------------------------------------------------------------------------------------------------------------ 3. auto-reset
def test_auto_reset_episodes_against_host_reads(kw):
    seen = set()
    for ckw, scale in (({}, 1.0), (copy.deepcopy(rc.FAIL_PRONE), 1.8), (copy.deepcopy(rc.EASY_SUCCESS), 1.0)):
        out = rc.run_auto_reset(kw, ckw, scale)
        seen |= out["terminations"]
        out["vec"].close()
    assert "steps" in seen and "success" in seen and len(seen - {"steps", "success"}) >= 1, seen


# ---------------------------------------------------------------------------------------------------- 4. store_derived off
@pytest.mark.parametrize("turbulence", [False, True])
def test_computed_derived_words_against_float64(kw, turbulence):
    worst = rc.run_derived_off(kw, turbulence)
    print("recorder, computed words 16..21 on the {}, turbulence {}: worst scaled error {:.3e} (bound {:.3e})".format(
        "emulation" if "_backend" in kw else "MI355X", turbulence, worst, DERIVED_BOUND))
    assert worst <= DERIVED_BOUND


# ----------------------------------------------------------------------------------------------------------- 6. host surface
def _flown(kw, n_steps=14, **vkw):
    cfg, ckw = _examples(steps_max=12)
    vec, rec = rc.vec_with_recorder(kw, cfg, ckw, **vkw)
    vec.reset()
    rng = np.random.default_rng(2)
    for _ in range(n_steps):
        vec.step(rng.uniform(-1, 1, size=(5, 3)).astype(np.float32))
    return vec, rec


def test_render_and_env_method(kw, tmp_path):
    pytest.importorskip("matplotlib")
    vec, rec = _flown(kw)
    assert rec.completed(0) == 1
    path = str(tmp_path / "render" / "direct.png")
    assert rec.render(save_path=path, show=False) is None and os.path.getsize(path) > 0
    path = str(tmp_path / "render" / "14")
    assert vec.env_method("render", indices=3, mode="plot", show=False, save_path=path + ".png") == [None]
    assert os.path.getsize(path + ".png") > 0
    assert vec.env_method("render", indices=1, show=False, save_path=path + "_untracked.png") == [None]     # not tracked
    assert not os.path.exists(path + "_untracked.png")
    vec.env_method("save_history", str(tmp_path / "h.npy"), ["roll"], indices=3)
    assert set(np.load(str(tmp_path / "h.npy"), allow_pickle=True).item()) == {"roll", "roll_target"}
    rec.detach()
    assert vec.env_method("render", indices=3, show=False, save_path=path + "_detached.png") == [None]      # as before the recorder
    assert not os.path.exists(path + "_detached.png")
    vec.close()


def test_no_render_before_the_first_episode_has_ended(kw, tmp_path):
    vec, rec = _flown(kw, n_steps=3)
    path = str(tmp_path / "early.png")
    assert vec.env_method("render", indices=3, show=False, save_path=path) == [None] and not os.path.exists(path)
    with pytest.raises(RuntimeError):
        rec.episode(0, "last")
    assert rec.episode(0, "current").length == 3
    vec.close()


def test_constructor_refusals_and_detach(kw):
    cfg, ckw = _examples(steps_max=12)
    vec = FixedWingVecEnv(cfg, num_envs=5, config_kw=ckw, **kw)
    for bad in ([5], [-1], [], list(range(5)) * 13):
        with pytest.raises(ValueError):
            FlightRecorder(vec, env_ids=bad)
    assert vec._recorder is None
    rec = FlightRecorder(vec, env_ids=[0, 4])
    with pytest.raises(RuntimeError):
        FlightRecorder(vec, env_ids=[1])
    assert rec.max_rows == 13 and rec.slot_of(4) == 1 and rec.slot_of(2) is None
    vec.reset()
    act = np.zeros((5, 3), np.float32)
    vec.step(act)
    before = np.array(vec._mem.to_host(rec.hdr))
    assert before[0, 1] == 2
    rec.detach()
    assert vec._recorder is None
    vec.step(act), vec.reset()
    np.testing.assert_array_equal(np.array(vec._mem.to_host(rec.hdr)), before)        # the header has stopped changing
    vec.close()
