"""Curriculum level changes in the middle of a run, on the host emulation of the unchanged kernel source (the GPU forms, eager
and under graph replay, are in tests/test_gpu_oracle_coverage.py): PPO.learn's CurriculumSchedule calls set_curriculum_level
between two rollouts, and from then on every reset has to draw from the new ranges -- although the step kernel has been
preparing every env's next reset draw, piece by piece, since its last reset.  What keeps a stale draw out is the tag
(configuration generation, episode) on every piece, read by the gym wave (`ready`), the physics wave (`pre_rows`), the piece
check of draw_stage_step and the per-env sets of k_model_draw, and bumped by fwg_update_config.  A wrong tag check resets an env
with the old ranges and nothing else happens: only a comparison with the oracle at the lanes concerned shows it
(coverage_runs.curriculum_sampled picks them: the classes of coverage_runs.curriculum_classes).

Two regimes.  DENSE: 45-step episodes of every age -- every wave hosts an end in most steps, so no prepared draw is ever
completed (curriculum_classes) and every reset draws on the spot: level changes against the restart of half-prepared pieces and
the never-ready path.  No mutant of the tag checks shows there, so it gets one rising run and, per kernel, the bit-identity of
a change to the level in force; its two-wave library is the one tests/test_emu_coverage.py builds.  SPARSE: 181-step episodes in six cohorts 30 steps apart, the changes on the step before a cohort's time
limit -- 60 % of the lanes hold a complete draw at a change, 30 % a half-prepared one, failures fall in between: the regime of a
real run (2 000-step episodes: 0.03 ends per wave and step), and the one in which a wrong tag check shows.

tools/mutation_check.py re-runs this file against kernel sources with each of the tag checks dropped (FWGYM_MUTANT_SRC /
FWGYM_MUTANT_TAG): all must fail here."""
import copy
import os
import time

import numpy as np
import pytest

import configs
import coverage_runs as cr
from emu.host_backend import HERE as EMU_DIR, HostBackend, build_emu, build_emu_spec
from gym_fixed_wing import presets
from gym_fixed_wing.config import EnvConfig
from gym_fixed_wing.vec_env import FixedWingVecEnv

MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")

TIGHT_ROLL_RATE = {"simulator": {"states": {6: {"constraint_min": -60, "constraint_max": 60}}}}
TURB = {"turbulence": True, "turbulence_intensity": "moderate"}
# (DENSE is the configuration of tests/test_emu_coverage.py: failure ends and time-limit ends in every launch)
REGIMES = {"dense": dict(steps_max=45, parts=None, n=256, window=96, chunk=16,
                         schedules={"rising": (0.25, {16: 0.57, 64: 1.0}), "falling": (1.0, {32: 0.3}), "same": (0.57, {32: 0.57})}),
           # cohorts reset at global steps 0, 30, .. 150 run out of time on window steps 30, 60, 90, .. (the window starts at 180):
           # the changes go before these steps, in the middle of a chunk
           "sparse": dict(steps_max=181, parts=6, n=384, window=120, chunk=16,
                          schedules={"rising": (0.25, {30: 0.57, 90: 1.0}), "falling": (1.0, {60: 0.3}), "same": (0.57, {60: 0.57})})}


def _ckw(regime, extra=None):
    return dict(copy.deepcopy(extra or {}), steps_max=REGIMES[regime]["steps_max"], **copy.deepcopy(TIGHT_ROLL_RATE))


def _generic_lib():
    """The emulation build whose kernels read every value from memory (a mutant: the same build of the mutated sources)."""
    if MUT_SRC is None:
        return build_emu()
    return build_emu(out=os.path.join(EMU_DIR, "libfwgym_emu{}.so".format(MUT_TAG)), src=MUT_SRC)


def _spec_lib(cfg, ckw, skw, rows, lean=True):
    ec = EnvConfig(copy.deepcopy(cfg), config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw))
    return build_emu_spec(ec, auto_reset=True, store_derived=not lean, obs_log_rows=rows, src=MUT_SRC, tag=MUT_TAG)


def _run(vec, cfg, ckw, skw, regime, schedule, what, **kw):
    t0 = time.time()
    R = REGIMES[regime]
    level0, changes = R["schedules"][schedule]
    what = "{} {} {}".format(what, regime, schedule)
    res = cr.curriculum_sampled(vec, cfg, ckw, skw, 11, level0, changes, window=R["window"], chunk=R["chunk"], parts=R["parts"],
                                sample=64, what=what, **kw)
    print(what, {k: v for k, v in res.items() if k != "buffers"}, "{:.0f} s".format(time.time() - t0))
    assert sorted(res["applied"].items()) == sorted(changes.items()), res["applied"]
    for s, counts in res["classes"].items():   # every class of lanes was among the checked, at every change
        for c in cr.CLASSES + (("a_ready", "c_ready", "half") if regime == "sparse" else ()):
            assert counts[c] >= (4 if c == "a_ready" else 1), (what, s, c, res["classes"])
    assert res["sampled_ends"] >= (100 if regime == "dense" else 50), res
    return res


def _plain_window(vec, level, regime, W):
    """The same run-in and window without any level change (the record of all envs)."""
    R = REGIMES[regime]
    vec.set_curriculum_level(level)
    run = cr._Run(vec, 8, 10)
    parts = R["parts"] or R["steps_max"]
    run.run_in(parts, R["steps_max"] // parts)
    run.alloc_window(W)
    for w in range(W):
        run.step_and_record(w)
    return {"done": np.asarray(run.done_b), "term": np.asarray(run.term_b), "reward": np.asarray(run.rew_b), "obs": np.asarray(run.obs_b)}


TWO_WAVE = [("dense", "row_log", "rising"), ("dense", "row_log", "same"), ("sparse", "row_log", "rising"), ("sparse", "dense", "falling")]


@pytest.mark.parametrize("regime,layout,schedule", TWO_WAVE, ids=["-".join(c) for c in TWO_WAVE])
def test_level_changes_on_the_two_wave_kernel_emulated(regime, layout, schedule):
    """k_step2 of the fail-prone cnn configuration: the gym wave's `ready`, the physics wave's `pre_rows` (a foreseen time-limit
    end whose complete draw belongs to the old generation must NOT be installed by the partner) and the piece check.  A change to
    the level in force moves the generation and not the ranges: bit for bit the run without the call."""
    cfg = configs.reference_like("cnn")
    ckw, skw = _ckw(regime, {"observation": {"step": 2}}), copy.deepcopy(TURB)
    rows = presets.OBS_LOG_ROWS if layout == "row_log" else 0
    n = REGIMES[regime]["n"]

    def make():
        return FixedWingVecEnv(copy.deepcopy(cfg), num_envs=n, config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw), seed=11,
                               derived_views=False, obs_log_rows=rows, _backend=HostBackend(), _lib_path=_spec_lib(cfg, ckw, skw, rows))
    vec = make()
    assert vec.spec_index == 0 and vec.obs_log_rows == rows        # the two-wave kernel k_step2 of this configuration
    res = _run(vec, cfg, ckw, skw, regime, schedule, "k_step2 " + layout, keep_buffers=schedule == "same")
    assert vec.spec_index == 0                                     # the ranges are read from memory: the instance stays
    if schedule == "same":
        vec2 = make()
        ref = _plain_window(vec2, REGIMES[regime]["schedules"]["same"][0], regime, res["window"])
        for k in ("done", "term", "reward", "obs"):
            assert np.array_equal(np.asarray(res["buffers"][k]), ref[k], equal_nan=True), k
        vec2.close()
    vec.close()


GENERIC = [("dense", "same"), ("sparse", "falling")]


@pytest.mark.parametrize("regime,schedule", GENERIC, ids=["-".join(c) for c in GENERIC])
def test_level_changes_on_the_generic_kernel_emulated(regime, schedule):
    """The default configuration (vector observation, one wave per 64 envs, every value from memory) with the tight roll-rate
    constraint."""
    cfg = configs.default()
    ckw = _ckw(regime)
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=REGIMES[regime]["n"], config_kw=copy.deepcopy(ckw), seed=11, _backend=HostBackend(),
                          _lib_path=_generic_lib())
    assert vec.spec_index == -1
    res = _run(vec, cfg, ckw, None, regime, schedule, "generic default", keep_buffers=schedule == "same")
    if schedule == "same":   # (the generation moves, the ranges do not: bit for bit the run without the call)
        vec2 = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=REGIMES[regime]["n"], config_kw=copy.deepcopy(ckw), seed=11, _backend=HostBackend(),
                               _lib_path=_generic_lib())
        ref = _plain_window(vec2, REGIMES[regime]["schedules"]["same"][0], regime, res["window"])
        for k in ("done", "term", "reward", "obs"):
            assert np.array_equal(np.asarray(res["buffers"][k]), ref[k], equal_nan=True), k
        vec2.close()
    vec.close()


PER_ENV = [("model_gaussian", "sparse", "rising"), ("reward_random_scaling", "sparse", "falling")]


@pytest.mark.parametrize("kind,regime,schedule", PER_ENV, ids=["-".join(c) for c in PER_ENV])
def test_level_changes_with_per_env_sets_emulated(kind, regime, schedule):
    """simulator.model / reward.randomize_scaling: every env's aircraft constants and reward scalings of its NEXT episode are
    prepared by k_model_draw / k_model_draw_q, tagged like the reset draw; a configuration update makes the host launch the
    full-grid draw once (model_all_stale), which must leave the run on the oracle's course.  (The level moves no range these
    sets are drawn from: a set kept across a level change is the set a new draw gives.  What its generation tag guards is the
    seed -- the test below.)"""
    cfg = configs.reference_like(kind)
    ckw = _ckw(regime)
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=REGIMES[regime]["n"], config_kw=copy.deepcopy(ckw), seed=11, _backend=HostBackend(),
                          _lib_path=_generic_lib())
    _run(vec, cfg, ckw, None, regime, schedule, kind)
    vec.close()


@pytest.mark.parametrize("kind", ["model_gaussian", "reward_random_scaling"])
def test_per_env_sets_prepared_under_another_seed_are_drawn_again_emulated(kind):
    """The smallest case in which the generation in the tags of k_model_draw matters: seed() in the middle of an episode.  The
    sets prepared for the next episode come from the old seed's streams; the reference draws at reset time, from the new one."""
    import parity
    cfg = configs.reference_like(kind)
    ckw = {"steps_max": 12}
    n = 6
    vec = FixedWingVecEnv(cfg, num_envs=n, config_kw=ckw, seed=3, as_numpy=True, _backend=HostBackend(), _lib_path=_generic_lib())
    orc = parity.make_oracles(cfg, n, 3, config_kw=ckw)
    np.testing.assert_allclose(vec.reset(), np.stack([o.reset() for o in orc]), atol=2e-5)
    acts = cr.jumpy_actions(9, 40, n)
    for t in range(40):
        if t == 8:     # (every env's next set was prepared right after the reset)
            vec.set_curriculum_level(0.3)
            for o in orc:
                o.set_curriculum_level(0.3)
        if t == 18:
            vec.seed(99)
            for i, o in enumerate(orc):
                o.seed(99)
                o.rng = parity.PhiloxStream(99, i)
                o.rng.begin_episode(o.simulator.episode)
        obs, rew, done, infos = vec.step(acts[t])
        for i, o in enumerate(orc):
            ob, r, d, info = o.step(acts[t][i].astype(np.float64))
            assert bool(done[i]) == d
            if d:
                ob = o.reset()
            np.testing.assert_allclose(obs[i], ob, rtol=4e-3, atol=4e-3, err_msg="step {} env {}".format(t, i))
            np.testing.assert_allclose(rew[i], r, rtol=4e-3, atol=4e-3, err_msg="reward, step {} env {}".format(t, i))
    vec.close()
