"""Oracle coverage of the regimes the benchmark advertises (round 6; the review of round 5: two wrong-answer bugs in terminal
observations had lived in the flagship kernel for five rounds because no oracle test ever entered these regimes).  All `-m gpu`,
all through the C ABI, all against oracle/ (float64 environments in a process pool, tests/oracle_pool.py):

  (a) the FROZEN preset kernels through their REAL time limit (steps_max = 2 000): k_step2<true, 6> (the benched instance,
      c3_cnn_step2_dryden_lean_log), <true, 7> (the same with derived host views), the dense <true, 4>, c2_default, c5_examples,
      and k_rollout (head + env step in one launch) of c5_examples_lean -- 96 envs x 2 080 steps, every value step() returns,
      the terminal observation, the nine metrics of a 2 000-step episode, the reset observation of the next one;
  (b) 65 536 envs in the bench's STEADY STATE (bench.py stagger_ages, then 300 steps): ~33 scattered time-limit ends, ~260
      early-episode lanes and ~190 draw pieces per launch; all outputs of all envs stay on the device (2 x 4.7 GB), 256 env ids
      are chosen AFTERWARDS from what happened and compared with oracles created by global env id under the same reset
      schedule -- row log and dense, the frozen benched kernels, and a fail-prone values-only variant on the shape instances
      (failure ends in every launch, steps that fail ON their time-limit step).

  (c) curriculum level changes in the middle of a run (PPO.learn's CurriculumSchedule between two rollouts), eager, under the
      replay of a captured graph of step calls, and as FusedRollout(graph=True) drives the env: 16 384 envs, the lanes on which a
      prepared reset draw of the old ranges would show picked AFTERWARDS (coverage_runs.curriculum_sampled / curriculum_classes);
      the replayed runs bit-identical to the eager ones; fwg_replay_check refusing exactly where the code says it must.

tools/mutation_check.py builds the kernels with round 5's two fixes reverted; FWGYM_MUTANT_LIB_ROW_LOG / _DENSE point (b)'s
fail-prone runs at them, and both mutants must fail there (profiles/r06_mutation_check.txt).  Its `hip` mode also builds the sparse-regime library of (c) with the
generation dropped from the prepared draw's tag checks (FWGYM_MUTANT_LIB_CURRICULUM points (c)'s sparse runs at it) and from
the per-env sets' (FWGYM_MUTANT_LIB_CURRICULUM_MODEL16: the c3_model16_lean_log runs)."""
import copy
import os
import time

import numpy as np
import pytest

import coverage_runs as cr
import oracle_pool as op
import parity
from gym_fixed_wing import _native as nat, presets
from gym_fixed_wing.vec_env import FixedWingVecEnv

pytestmark = pytest.mark.gpu
SEED = int(os.environ.get("FWGYM_COV_SEED", "11"))   # (another seed = other initial states, targets, turbulence, reset draws: a hunt)

# Absolute tolerance of the runs through 2 000-step episodes (relative: 4e-3 as everywhere).  The airspeed target of class
# `compensate` (fixed_wing.py:944-972) is INTEGRATED over the episode with a slope that switches on thresholds of the target
# itself: in float32 a switch can fall one step later than in float64, and the two targets then differ by one increment
# (0.0064 m/s, measured, emulator and GPU alike) until the next switch -- visible in the observation's target-error entries.
# Round 5's bugs are 0.06 m/s (air data) and O(1) (lagged rows); the short-episode runs keep 4e-3.
LONG_ATOL = 1.5e-2

FROZEN = ["c3_cnn_step2_dryden_lean_log", "c3_cnn_step2_dryden_log", "c3_cnn_step2_dryden_lean", "c2_default", "c5_examples"]


def _preset(name):
    _, kind, ckw, skw = [e for e in presets.SPECIALISED if e[0] == name][0]
    return presets.preset(kind), copy.deepcopy(ckw), copy.deepcopy(skw)


def _make(name, n, **kw):
    cfg, ckw, skw = _preset(name)
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=n, device=0, config_kw=ckw, sim_config_kw=skw, seed=SEED,
                          derived_views="_lean" not in name, obs_log_rows=presets.OBS_LOG_ROWS if name.endswith("_log") else 0, **kw)
    assert vec.spec_index == [e[0] for e in presets.SPECIALISED].index(name), (name, vec.spec_index)   # the frozen kernel itself
    assert int(vec.cfg["steps_max"]) == 2000
    return vec, cfg, ckw, skw


@pytest.mark.parametrize("name", FROZEN)
def test_frozen_preset_through_its_real_time_limit(name):
    t0 = time.time()
    vec, cfg, ckw, skw = _make(name, 96, as_numpy=True)
    res = cr.through_time_limit(vec, cfg, ckw, skw, SEED, 2080, atol=LONG_ATOL, what=name)
    print(name, res, "{:.0f} s".format(time.time() - t0))
    assert res["episodes"] >= 96 and res["terminations"].get("steps", 0) >= 80, res
    vec.close()


def test_one_launch_rollout_step_through_the_time_limit():
    """k_rollout of c5_examples_lean (policy head + env step in ONE launch, fwg_rollout_step): the env half against oracles fed
    with the actions the head sampled -- raw observation, reward, done, termination, terminal observation -- through 2 000-step
    time limits.  The head itself is compared with torch in tests/test_actor.py / test_rollout.py."""
    import torch
    from gym_fixed_wing.actor import DeviceActor
    from gym_fixed_wing.rollout import FusedRollout, MlpPolicy
    name = "c5_examples_lean"
    vec, cfg, ckw, skw = _make(name, 96)
    N, D, T, chunk = vec.num_envs, vec.obs_dim, 2080, 16
    torch.manual_seed(0)
    policy = MlpPolicy(D)
    with torch.no_grad():
        policy.log_std.fill_(-1.2)      # (a random-init policy with unit noise tumbles the aircraft within a second)
    actor = DeviceActor.for_env(vec, seed=7)
    actor.load_policy(policy)
    rec = {"obs": np.zeros((T, N, D)), "reward": np.zeros((T, N)), "done": np.zeros((T, N), dtype=bool), "target": np.zeros((T, N, 3)),
           "term": {}, "term_obs": {}, "metrics": {}, "masked_reset_obs": {}, "anchors": {}}
    acts = np.zeros((T, N, 3), dtype=np.float32)
    rec["reset_obs"] = parity._np(vec.reset()).reshape(N, D).astype(np.float64)
    state = {"base": 0}

    def tap(t, o, r, d):
        g = state["base"] + t
        rec["obs"][g], rec["reward"][g] = parity._np(o).reshape(N, D), parity._np(r)
        dn = parity._np(d).astype(bool)
        rec["done"][g] = dn
        if dn.any():
            term, tobs = parity._np(vec._term), parity._np(vec._term_obs)
            for i in np.nonzero(dn)[0]:
                rec["term"][(g, int(i))] = nat.term_name(term[i])
                rec["term_obs"][(g, int(i))] = tobs[i].astype(np.float64).reshape(-1)
        if g % 250 == 249:
            rec["anchors"][g] = op.sim_rows(vec)

    ro = FusedRollout(vec, actor, chunk, graph=False, fused=True, tap=tap)
    assert ro.fused
    for c in range(T // chunk):
        state["base"] = c * chunk
        buf = ro.run()
        acts[c * chunk:(c + 1) * chunk] = parity._np(buf["actions"])
    tr = op.run_traces(copy.deepcopy(cfg), list(range(N)), acts, SEED, config_kw=ckw, sim_config_kw=skw, anchors=rec["anchors"])
    res = op.compare(rec, tr, 4e-3, LONG_ATOL, what="k_rollout " + name, check_target=False)
    print("k_rollout", name, res)
    assert res["episodes"] >= N, res
    vec.close()


# ----------------------------------------------------------------------------------------------------------------------
FAIL_PRONE_CKW = {"steps_max": 45, "simulator": {"states": {6: {"constraint_min": -60, "constraint_max": 60}}}}


@pytest.mark.parametrize("layout", ["row_log", "dense"])
@pytest.mark.parametrize("variant", ["frozen", "fail_prone", "fail_prone_lockstep"])
def test_steady_state_of_65536_envs_sampled_against_oracles(variant, layout):
    t0 = time.time()
    n = 65536
    cfg, ckw, skw, _, _ = presets.workload("c3")
    rows = presets.OBS_LOG_ROWS if layout == "row_log" else 0
    kw = {}
    if variant != "frozen":
        ckw = dict(copy.deepcopy(ckw), **copy.deepcopy(FAIL_PRONE_CKW))
        mutant = os.environ.get("FWGYM_MUTANT_LIB_" + layout.upper())
        kw = {"_lib_path": mutant} if mutant else {"specialize": False}
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=n, device=0, config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw), seed=SEED,
                          derived_views=False, obs_log_rows=rows, **kw)
    want = [e[0] for e in presets.SPECIALISED].index("c3_cnn_step2_dryden_lean_log" if rows else "c3_cnn_step2_dryden_lean")
    if variant == "frozen":
        assert vec.spec_index == want                                   # k_step2<true, 6> / <true, 4>: the benched instances
    elif "_lib_path" not in kw:
        assert vec.spec_index == nat.INSTANCE_SHAPE + want, vec.spec_index   # their shape instances (values from memory)
    res = cr.steady_state_sampled(vec, cfg, ckw, skw, SEED, window=300, sample=256, parts=0 if variant.endswith("lockstep") else None,
                                  atol=LONG_ATOL if variant == "frozen" else 4e-3,
                                  what="steady state, {} envs, {} {}".format(n, variant, layout))
    print(variant, layout, res, "{:.0f} s".format(time.time() - t0))
    per_step = res["ends_in_window"] / 300.0
    if variant == "frozen":
        assert 20 <= per_step <= 60, per_step                           # (65 536 / 2 000 = 33 ends per launch)
        assert res["sampled_ends"] >= 64, res
    else:
        assert res["failure_ends"] >= 10000 and res["failed_on_the_limit_step_checked"] >= 32, res
    vec.close()


@pytest.mark.parametrize("regime", ["staggered", "lockstep"])
def test_shipped_cnn_configuration_failed_steps_on_the_log_s_wrap_step(regime):
    """The shipped cnn configuration (5 rows at step 1, row log) with a tight roll-rate constraint, on its shape instance: a step
    that fails on a wrap step of the row log (every 32nd global step) shows the record of five steps ago in its terminal
    observation's oldest row -- one further back than the four rows the wrap carries.  Rounds 1-5 read it one plane past the log
    (found by tests/test_emu_fuzz.py in round 6; tools/mutation_check.py mutant `log_plane_past_the_log`).  The lanes that failed
    on a wrap step are picked first."""
    t0 = time.time()
    n = 65536
    cfg = presets.preset("cnn")
    ckw = copy.deepcopy(FAIL_PRONE_CKW)
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=n, device=0, config_kw=copy.deepcopy(ckw), seed=SEED, specialize=False)
    want = [e[0] for e in presets.SPECIALISED].index("ship_cnn_log")
    assert vec.spec_index == nat.INSTANCE_SHAPE + want and vec.obs_log_rows == presets.OBS_LOG_ROWS and vec.obs_window_period == 32

    def on_wrap(fail_ends, steps_ends, g0):
        w = np.arange(fail_ends.shape[0])
        rows = fail_ends[(g0 + w) % 32 == 0]
        return np.nonzero(rows.any(axis=0))[0]

    res = cr.steady_state_sampled(vec, cfg, ckw, None, SEED, window=200, sample=256, first_pick=on_wrap, parts=0 if regime == "lockstep" else None,
                                  what="shipped cnn configuration, fail-prone, {} envs, {}".format(n, regime))
    print("ship_cnn", res, "{:.0f} s".format(time.time() - t0))
    assert res["first_pick_checked"] >= 32 and res["failure_ends"] >= 10000, res
    vec.close()


# ----------------------------------------------------------------------------------------------------------------------
# the other frozen configurations: every shipped configuration file + the randomised-aircraft workload, on their SHAPE instances
# with fail-prone values (45-step episodes, tight roll-rate constraint), in both regimes -- the two-wave kernel's episode-end
# machinery with vector observations (dense batch, attached-less), the mlp variant's unscaled actions, per-env aircraft constants
SWEEP = [("c2_default", "default", None, None, True), ("c5_examples", "examples", None, None, True), ("ship_mlp", "mlp", None, None, True),
         ("c3_model16_lean_log", "cnn_model16", {"observation": {"step": 2}}, dict(presets.TURB_MODERATE), False)]


@pytest.mark.parametrize("regime", ["staggered", "lockstep"])
@pytest.mark.parametrize("entry", SWEEP, ids=[e[0] for e in SWEEP])
def test_preset_shape_instances_fail_prone_against_oracles(entry, regime):
    t0 = time.time()
    name, kind, ckw0, skw, derived = entry
    n = 16384
    cfg = presets.preset(kind)
    ckw = dict(copy.deepcopy(ckw0 or {}), **copy.deepcopy(FAIL_PRONE_CKW))
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=n, device=0, config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw), seed=SEED,
                          derived_views=derived, specialize=False)
    want = [e[0] for e in presets.SPECIALISED].index(name)
    assert vec.spec_index == nat.INSTANCE_SHAPE + want, (name, vec.spec_index)
    res = cr.steady_state_sampled(vec, cfg, ckw, skw, SEED, window=200, sample=192, parts=0 if regime == "lockstep" else None,
                                  what="{} shape instance, fail-prone, {} envs, {}".format(name, n, regime))
    print(name, regime, res, "{:.0f} s".format(time.time() - t0))
    assert res["failure_ends"] >= 1000 and res["time_limit_ends"] >= 1000 and res["sampled_ends"] >= 200, res
    vec.close()


# ----------------------------------------------------------------------------------------------------------------------
# (c) curriculum level changes in the middle of a run
# ----------------------------------------------------------------------------------------------------------------------
RISING = (0.25, {32: 0.57, 96: 1.0})          # {window step: level}, chunks of 32 steps
# the sparse regime of tests/test_emu_curriculum.py: 181-step episodes in six cohorts 30 steps apart, which run out of time on the
# window steps 30, 60, 90, ..; the changes before steps 30 and 90, chunks of 30 steps
SPARSE_CKW = dict(copy.deepcopy(FAIL_PRONE_CKW), steps_max=181)
CURRICULUM_CASES = {
    # name: (preset kind, config_kw, sim_config_kw, derived views, row log, frozen preset it starts on | preset whose shape instance
    #        it runs, atol, parts, window, (level0, schedule), per-env sets, chunk)
    "c5_examples": ("examples", None, None, True, False, "c5_examples", None, LONG_ATOL, None, 160, RISING, False, 32),
    "c3_fail_prone_log": ("cnn", dict({"observation": {"step": 2}}, **copy.deepcopy(FAIL_PRONE_CKW)), dict(presets.TURB_MODERATE), False, True,
                          None, "c3_cnn_step2_dryden_lean_log", 4e-3, None, 160, RISING, False, 32),
    "c3_model16_lean_log": ("cnn_model16", dict({"observation": {"step": 2}}, **copy.deepcopy(FAIL_PRONE_CKW)), dict(presets.TURB_MODERATE), False,
                            True, None, "c3_model16_lean_log", 4e-3, None, 160, RISING, True, 32),
    "c3_sparse_log": ("cnn", dict({"observation": {"step": 2}}, **copy.deepcopy(SPARSE_CKW)), dict(presets.TURB_MODERATE), False, True,
                      None, "c3_cnn_step2_dryden_lean_log", 4e-3, 6, 150, (0.25, {30: 0.57, 90: 1.0}), False, 30),
}
N_CURRICULUM = 16384


def _curriculum_env(case):
    kind, ckw, skw, derived, log, frozen, shape_of, atol, parts, window, schedule, per_env, chunk = CURRICULUM_CASES[case]
    cfg = presets.preset(kind)
    kw = {}
    names = [e[0] for e in presets.SPECIALISED]
    if frozen is None:
        mutant = os.environ.get({"c3_sparse_log": "FWGYM_MUTANT_LIB_CURRICULUM", "c3_model16_lean_log": "FWGYM_MUTANT_LIB_CURRICULUM_MODEL16"}.get(case, "-"))
        kw = {"_lib_path": mutant} if mutant else {"specialize": False}
    vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=N_CURRICULUM, device=0, config_kw=copy.deepcopy(ckw), sim_config_kw=copy.deepcopy(skw),
                          seed=SEED, derived_views=derived, obs_log_rows=presets.OBS_LOG_ROWS if log else 0, **kw)
    if frozen is not None:
        assert vec.spec_index == names.index(frozen), (case, vec.spec_index)                 # the frozen kernel itself
    elif "_lib_path" not in kw:
        assert vec.spec_index == nat.INSTANCE_SHAPE + names.index(shape_of), (case, vec.spec_index)   # its shape instance
    return vec, cfg, ckw, skw


def _print_curriculum(what, res, t0):
    print(what, {k: v for k, v in res.items() if k != "buffers"}, "{:.0f} s".format(time.time() - t0))


def _check_curriculum_counts(case, res):
    for s, c in res["classes"].items():
        if case in ("c3_fail_prone_log", "c3_model16_lean_log", "c3_sparse_log"):   # the fail-prone cases
            assert c["a"] >= 32 and c["c"] >= 32 and c["b"] >= 8 and c["d"] >= 8, (case, s, c)
        if case == "c3_sparse_log":   # ... and where prepared draws are completed: lanes that HELD a complete / a half-prepared one
            assert c["a_ready"] >= 32 and c["c_ready"] >= 16 and c["half"] >= 8, (case, s, c)


@pytest.mark.parametrize("case", list(CURRICULUM_CASES))
def test_curriculum_level_changes_eager_against_oracles(case):
    """set_curriculum_level between chunks of direct steps, 0.25 -> 0.57 -> 1.0; 256 env ids chosen afterwards.
    Counts are asserted in the fail-prone cases.  c5_examples (2 000-step episodes: 8 of 16 384 lanes at their time limit per
    step, failures rare) asserts none; what it reaches is printed with the summary and has not been recorded from a GPU run yet
    (profiles/gpu_suite_durations.txt lists it as outstanding)."""
    t0 = time.time()
    vec, cfg, ckw, skw = _curriculum_env(case)
    _, _, _, _, _, _, _, atol, parts, window, (level0, schedule), _, chunk = CURRICULUM_CASES[case]
    inst = vec.spec_index
    res = cr.curriculum_sampled(vec, cfg, ckw, skw, SEED, level0, schedule, window=window, chunk=chunk, sample=256, parts=parts, atol=atol,
                                what="curriculum, eager, " + case)
    _print_curriculum("curriculum eager " + case, res, t0)
    assert vec.spec_index == inst                      # (the level moves no folded value: the instance stays)
    assert sorted(res["applied"]) == sorted(schedule)
    _check_curriculum_counts(case, res)
    vec.close()


@pytest.mark.parametrize("case", list(CURRICULUM_CASES))
def test_curriculum_level_changes_under_graph_replay(case):
    """The same runs with the window driven by a captured graph of 32 (30) step_device calls (coverage_runs.ReplayedChunks), the level
    changed between replays.  fwg_replay_check refuses exactly where the code says it must: never for the instance (a level
    change leaves it), at every change for a configuration with per-env parameter sets (simulator.model: which draw kernel a
    step launches is decided on the host) -- there the recipe of its message, two direct steps and a new capture.  Bit-identical
    to the eager run of the same chunks over ALL envs, and compared with the oracles."""
    t0 = time.time()
    _, _, _, _, _, _, _, atol, parts, window, (level0, schedule), per_env, chunk = CURRICULUM_CASES[case]
    vec, cfg, ckw, skw = _curriculum_env(case)
    inst = vec.spec_index
    stepper = cr.ReplayedChunks(vec, chunk)
    res = cr.curriculum_sampled(vec, cfg, ckw, skw, SEED, level0, schedule, window=window, chunk=chunk, stepper=stepper, sample=256, parts=parts,
                                atol=atol, what="curriculum, replayed, " + case, keep_buffers=True)
    _print_curriculum("curriculum replayed " + case, res, t0)
    print("refusals", stepper.refusals, "captures", stepper.captures)
    assert vec.spec_index == inst and set(stepper.instances) == {inst}
    applied = sorted(res["applied"])
    assert len(applied) == len(schedule)
    if per_env:
        assert [w for w, _ in stepper.refusals] == applied and stepper.captures == 1 + len(applied), (stepper.refusals, applied)
        assert all("per-env" in msg and "another kernel instance" not in msg for _, msg in stepper.refusals), stepper.refusals
    else:
        assert stepper.refusals == [] and stepper.captures == 1, stepper.refusals
    _check_curriculum_counts(case, res)
    rep = res["buffers"]
    vec.close()
    # ---- the eager run of the same chunks and the same changes
    vec2, _, _, _ = _curriculum_env(case)
    res2 = cr.curriculum_sampled(vec2, cfg, ckw, skw, SEED, level0, res["applied"], window=res["window"], chunk=res["chunks"], sample=256,
                                 parts=parts, keep_buffers=True, compare=False)
    eag = res2["buffers"]
    assert res2["window"] == res["window"] and res2["applied"] == res["applied"]
    done = rep["done"] != 0
    for k in ("done", "term", "reward", "obs"):
        a, b = rep[k], eag[k]
        same = (a == b) | ((a != a) & (b != b)) if a.dtype.is_floating_point else (a == b)
        assert bool(same.all()), "{}: {} of {} values differ between the replayed and the eager run, first at {}".format(
            k, int((~same).sum()), same.numel(), (~same).nonzero()[0].tolist())
    a, b = rep["term_obs"][done], eag["term_obs"][done]
    assert bool(((a == b) | ((a != a) & (b != b))).all()), "terminal observations differ"
    print("replayed == eager over all envs: {} steps x {} envs, {} ends; {:.0f} s".format(res["window"], N_CURRICULUM, int(done.sum()), time.time() - t0))
    vec2.close()


def test_curriculum_level_changes_as_the_learner_drives_them():
    """FusedRollout(graph=True) under a DeviceActor on c5_examples, as PPO.learn runs it: the level is changed between run() calls
    and the rollout is captured anew under ppo.py's rule (the instance moved) -- which a level change never meets, so the ONE graph
    captured at the start is replayed throughout (replay_check inside run()).  The second change comes 13 steps before the
    cohort's time limit: every lane that is still in its first episode holds a complete draw of the old ranges.  Oracles of env
    ids chosen afterwards, fed buf["actions"]: buf["dones"] at every step, the raw observation at every chunk end."""
    import torch
    from gym_fixed_wing.actor import DeviceActor
    from gym_fixed_wing.rollout import FusedRollout, MlpPolicy
    t0 = time.time()
    name = "c5_examples"
    vec, cfg, ckw, skw = _make(name, N_CURRICULUM)
    N, D, chunk, C = vec.num_envs, vec.obs_dim, 16, 132
    changes = {40: 0.57, 124: 1.0}                  # {chunk index: level}: before global steps 642 and 1 986 (time limit: step 1 999)
    T = 2 + chunk * C                               # (the capture's warm-up makes two steps of its own)
    torch.manual_seed(0)
    policy = MlpPolicy(D)
    with torch.no_grad():
        policy.log_std.fill_(-1.2)
    actor = DeviceActor.for_env(vec, seed=7)
    actor.load_policy(policy)
    vec.set_curriculum_level(0.25)
    reset_obs = vec.reset().reshape(N, D).clone()
    dev = reset_obs.device
    acts, dones = torch.zeros((T, N, 3), device=dev), torch.zeros((T, N), dtype=torch.uint8, device=dev)
    obs_end, rows_at = {}, {}
    warm = []
    step_device = vec.step_device

    def spy(a, want_obs=True):   # the two warm-up steps of the capture belong to the env's life: their actions and dones
        out = step_device(a, want_obs=want_obs)
        if not torch.cuda.is_current_stream_capturing():
            warm.append((a.clone(), out[2].clone()))
        return out

    vec.step_device = spy
    ro = FusedRollout(vec, actor, chunk, graph=True)
    vec.step_device = step_device
    torch.cuda.synchronize()
    assert len(warm) == 2, len(warm)
    for t, (a, d) in enumerate(warm):
        acts[t], dones[t] = a, d
    spec_at_capture, captures = vec.spec_index, 1
    g = 2
    for c in range(C):
        if c in changes:
            vec.set_curriculum_level(changes[c])
            if vec.spec_index != spec_at_capture:   # (ppo.py's rule)
                ro = FusedRollout(vec, actor, chunk, graph=True)
                spec_at_capture, captures = vec.spec_index, captures + 1
        buf = ro.run()
        acts[g:g + chunk], dones[g:g + chunk] = buf["actions"], buf["dones"]
        g += chunk
        obs_end[g - 1] = vec._obs.reshape(N, D).clone()
        if g % 256 < chunk:
            rows_at[g - 1] = cr._clone(cr._sim_rows(vec))
    torch.cuda.synchronize()
    assert captures == 1 and g == T
    done_h = dones.cpu().numpy().astype(bool)
    # ---- env ids: lanes that failed after a change (their reset is an unforeseen one), lanes at their time limit, uniform picks
    sel = np.random.default_rng(0)
    ends_after = done_h[2 + chunk * 40:].sum(axis=0)
    early = np.nonzero(done_h[2 + chunk * 40:1999].any(axis=0))[0]
    pos = list(sel.choice(early, size=min(40, len(early)), replace=False))
    rest = [int(e) for e in sel.permutation(N) if int(e) not in set(int(p) for p in pos)]
    pos = np.array(sorted(int(p) for p in pos) + rest[:96 - len(pos)])
    pos.sort()
    ti = torch.as_tensor(pos, device=dev)
    anchors = {}
    for gs, rows in rows_at.items():
        w_ = rows[:, ti].cpu().numpy().astype(np.float64).transpose(1, 0, 2).reshape(len(pos), 32)
        anchors[gs] = (w_[:, :18].copy(), w_[:, 18:26].copy(), w_[:, 26:32].copy())
    curriculum = {-1: 0.25}
    curriculum.update({2 + chunk * c: lvl for c, lvl in changes.items()})
    tr = op.run_traces(copy.deepcopy(cfg), [int(p) for p in pos], acts[:, ti].cpu().numpy(), SEED, config_kw=ckw, sim_config_kw=skw,
                       anchors=anchors, curriculum=curriculum)
    worst = float(np.abs(reset_obs[ti].cpu().numpy() - tr["reset_obs"]).max())
    assert worst <= 4e-3, worst
    dd = done_h[:, pos] != tr["done"]
    first_bad = np.where(dd.any(axis=0), np.argmax(dd, axis=0), T)
    differing = [(int(first_bad[j]), int(pos[j]), tr["term"].get((int(first_bad[j]), j))) for j in np.nonzero(dd.any(axis=0))[0]]
    # (a constraint comparison within float32 rounding of the limit: oracle_pool.compare's max_borderline; never a time-limit end)
    assert len(differing) <= 2 and all(name != "steps" for _, _, name in differing), differing
    checked = 0
    for gs, ob in sorted(obs_end.items()):
        got, want = ob[ti].cpu().numpy().astype(np.float64), tr["obs"][gs]
        ok = gs < first_bad
        err = np.abs(got - want)[ok]
        tol = (LONG_ATOL + 4e-3 * np.abs(want))[ok]
        assert (err <= tol).all(), "raw observation at step {}: worst |d| {:.3e}, env {}".format(
            gs, err.max(), pos[ok][np.argmax((err - tol).max(axis=1))])
        worst = max(worst, float(err.max()) if err.size else 0.0)
        checked += int(ok.sum())
    at_limit = int(done_h[1999, pos].sum())
    print("learner-driven c5_examples: {} env ids, {} episodes ({} at the time limit 13 steps after the second change, {} of the ids ended "
          "after the first change), {} chunk-end observations, worst |d| {:.3e}, done differs {}; {:.0f} s".format(
              len(pos), int(tr["done"].sum()), at_limit, int((ends_after[pos] > 0).sum()), checked, worst, differing, time.time() - t0))
    assert at_limit >= 40 and int(tr["done"].sum()) >= len(pos), (at_limit, int(tr["done"].sum()))
    vec.close()


def test_curriculum_level_change_at_the_time_limit_of_2000_step_episodes():
    """The benched c3_cnn_step2_dryden_lean_log in lock-step: one change, 1.0 -> 0.3, before step 1 999 -- the step on which the
    cohort runs out of time, in the middle of a chunk: the gym wave has foreseen every one of these ends, every lane holds a
    complete draw of the old ranges, and the physics wave must NOT install it.  SCOPE: the window goes on for 95 steps after the
    change, so of the first episode after the change of every sampled env the reset observation and its first 95 steps are
    compared, at LONG_ATOL, not all 2 000 -- a draw of the wrong ranges shows in the reset observation itself, and the rest of a
    2 000-step episode is what test_frozen_preset_through_its_real_time_limit runs; the whole episode would keep 2 000 more
    steps of 16 384 envs on the device and double the oracles' time against the suite's 900 s ceiling."""
    t0 = time.time()
    name = "c3_cnn_step2_dryden_lean_log"
    vec, cfg, ckw, skw = _make(name, N_CURRICULUM)
    res = cr.curriculum_sampled(vec, cfg, ckw, skw, SEED, 1.0, {99: 0.3}, window=192, chunk=32, sample=128, parts=0, run_in_steps=1900,
                                atol=LONG_ATOL, what="curriculum at the time limit, " + name)
    _print_curriculum("curriculum at the time limit " + name, res, t0)
    c = res["classes"][99]
    assert res["applied"] == {99: 0.3} and 32 in res["chunks"] and 3 in res["chunks"], res["chunks"]   # (96 + 3: not chunk-aligned)
    assert c["a_ready"] >= 32 and c["a_ready_all"] >= N_CURRICULUM // 2, c
    assert res["sampled_ends"] >= 128, res
    vec.close()
