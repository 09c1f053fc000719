"""The evaluation protocol on the device (include/fwgym.h "Evaluation": fwg_pid_act, fwg_eval_advance;
gym_fixed_wing.evaluate.evaluate_on_set_device) on the HOST EMULATION of the kernels -- the CPU half of the suite; the GPU half
is tests/test_eval_device_gpu.py and shares its inputs and yardsticks (tests/eval_device_common.py).

  tracker    against a twenty-line numpy restatement, exactly: wave and workgroup tails, an env done at step 0, envs reporting
             done again with other term codes / metrics columns, NaN rewards and NaN action rows, sentinels behind every buffer;
  PID head   against oracle.pyfly_restated.PIDController in float64, open loop, non-default gains (all eight non-zero), strided
             and permuted columns; bound: twice the error of the torch fp32 BatchedPID on the same inputs (at most 1e-3);
  protocol   five shipped scenarios against the float64 oracle env + its scalar PID (the comparison of tests/test_evaluate.py);
  host reads at most one per chunk of steps."""
import json
import os

import numpy as np
import pytest

import configs
import eval_device_common as edc
from emu.host_backend import HERE as EMU_HERE, HostBackend, build_emu as _build_emu
from gym_fixed_wing import _native as nat
from gym_fixed_wing import evaluate as ev
from oracle.gym_restated import FixedWingOracle
from oracle.pyfly_restated import PIDController

HERE = os.path.dirname(os.path.abspath(__file__))
# tools/mutation_check.py re-runs this file against kernel sources with a bug put in (the eval_* mutants)
MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")


def build_emu():
    return _build_emu(src=MUT_SRC, out=os.path.join(EMU_HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else _build_emu()


@pytest.fixture(scope="module")
def emu():
    return nat.load_library(build_emu()), HostBackend()


def _scenarios():
    with open(os.path.join(HERE, "golden", "test_set_wind_none.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("n", edc.TRACKER_N)
def test_tracker_matches_the_numpy_restatement_exactly(emu, n):
    got, want, sentinels = edc.run_tracker(*emu, n)
    edc.assert_tracker(got, want, sentinels)


def test_tracker_script_holds_the_cases_that_matter():
    """The scripted inputs themselves: an env done at step 0, envs that never end, envs whose later dones carry other term codes
    and other metrics columns than the first, NaN rewards / action rows of ended envs."""
    reward, done, term, metrics, actions = edc.tracker_inputs(65)
    want = edc.tracker_reference(reward, done, term, metrics, actions, -7.0)
    assert (want["length"] == 1).any() and (want["active"] == 1).any()
    first = np.argmax(done, axis=0)
    again = [(e, t) for e in range(65) for t in range(first[e] + 1, done.shape[0]) if done[first[e], e] and done[t, e]]
    assert len(again) >= 13
    assert all(term[t, e] != term[first[e], e] or not np.array_equal(metrics[t, :, e], metrics[first[e], :, e]) for e, t in again)
    assert all(not np.array_equal(metrics[t, :, e], metrics[first[e], :, e]) for e, t in again)
    assert any(term[t, e] != term[first[e], e] for e, t in again)
    ended = np.cumsum(done, axis=0) > 0
    assert np.isnan(actions[1:][ended[:-1]]).all() and np.isnan(reward[1:][ended[:-1]]).all() and ended[:-1].any()
    assert (want["metrics_final"][:, want["active"] == 1] == -7.0).all()      # never done: the column stays the caller's


def test_tracker_and_pid_refuse_bad_arguments(emu):
    for out in (edc.tracker_refusals(*emu), edc.pid_refusals(*emu)):
        for name, (status, msg) in out.items():
            assert status == -1, name                                   # FWG_ERR_INVALID
            assert msg.startswith("fwg_"), (name, msg)


@pytest.mark.parametrize("n", edc.PID_N)
def test_pid_head_against_float64(emu, n):
    acts, integ, inp = edc.run_pid(*emu, n)
    edc.assert_pid_inputs_exercise_every_term(inp)
    err = edc.pid_errors(acts, integ, inp)
    print("fwg_pid_act on the emulation, N = {}: {}".format(n, {k: "%.3g" % v for k, v in err.items()}))
    assert edc.PID_BOUND <= 1e-3
    for k, v in err.items():
        assert v <= edc.PID_BOUND, (k, v, edc.PID_BOUND)


def test_the_asserted_bound_is_twice_the_torch_baselines_error():
    """PID_BOUND is a constant (profiles/pid_head_errors.txt); here the measurement it came from is repeated, so that inputs and
    constant cannot drift apart: the parent's BatchedPID in torch fp32 on the CPU stays within the recorded worst figure, up to the
    10 % that another torch build's sin / cos may move it."""
    worst = max(max(edc.pid_errors(*edc.pid_torch_fp32(edc.pid_inputs(n)), edc.pid_inputs(n)).values()) for n in edc.PID_N)
    assert 0.5 * edc.PID_TORCH_WORST <= worst <= 1.1 * edc.PID_TORCH_WORST, worst


def _oracle_eval(scenarios, cfg):
    """The protocol on the float64 oracle env with its scalar PID (restated from tests/test_evaluate.py)."""
    kw = ev.evaluation_overrides(True)
    out = []
    for sc in scenarios:
        env = FixedWingOracle(cfg, config_kw=kw, sim_config_kw={"turbulence": False, "turbulence_intensity": "none"})
        obs = env.reset(state=sc["state"], target=sc["target"])
        pid = PIDController(env.simulator.dt)
        pid.set_reference(sc["target"]["roll"], sc["target"]["pitch"], sc["target"]["Va"])
        rews, done, info = [], False, None
        while not done:
            if info is not None:
                pid.set_reference(info["target"]["roll"], info["target"]["pitch"], info["target"]["Va"])
            obs, r, done, info = env.step(pid.get_action(obs[0], obs[1], obs[2], obs[3:6]))
            rews.append(r)
        out.append((rews, info))
    return out


@pytest.fixture(scope="module")
def five():
    cfg = configs.reference_like("examples")
    scen = _scenarios()[:5]
    return cfg, scen, ev.evaluate_on_set_device(scen, cfg, _backend=HostBackend(), _lib_path=build_emu())


def test_pid_protocol_matches_oracle_on_emulated_kernels(five):
    cfg, scen, result = five
    res = result.as_reference_layout()
    want = _oracle_eval(scen, cfg)
    for i, (rews, info) in enumerate(want):
        assert abs(len(res["rewards"][i]) - len(rews)) <= 1, (i, len(res["rewards"][i]), len(rews))
        n = min(len(rews), len(res["rewards"][i]))
        np.testing.assert_allclose(res["rewards"][i][:n], rews[:n], atol=5e-3)
        assert res["termination"][i] == info["termination"] == "success"
        assert bool(res["success"]["all"][i]) is True
        for k in ("roll", "pitch", "Va"):
            assert abs(res["settling_time"][k][i] - info["settling_time"][k]) <= 1
    table = result.table()
    assert table["success_%"]["all"] == 100.0 and 1.0 < table["settling_time"]["roll"] < 3.5


def test_result_layouts_agree_with_the_host_loop(five):
    """as_reference_layout() has the layout of evaluate_on_set's dict and table() gives exactly the numbers of summarize() on it.
    Against the host loop itself the PID path agrees up to the rounding between BatchedPID's torch arithmetic and the kernel's (the
    head path, same kernel on both sides, is compared bit for bit on the GPU)."""
    cfg, scen, result = five
    host = ev.evaluate_on_set(scen, cfg, as_numpy=True, _backend=HostBackend(), _lib_path=build_emu())
    res = result.as_reference_layout()
    assert set(res) == set(host)
    assert res["termination"] == host["termination"]
    assert [len(r) for r in res["rewards"]] == [len(r) for r in host["rewards"]] == list(result.length)
    assert res["success"] == host["success"]
    for m in ev.METRICS:
        assert set(res[m]) == set(host[m]), m
        for state in res[m]:
            assert [type(x) for x in res[m][state]] == [type(x) for x in host[m][state]], (m, state)
            np.testing.assert_allclose(np.array(res[m][state], dtype=np.float64), np.array(host[m][state], dtype=np.float64),
                                       rtol=1e-5, err_msg="{} {}".format(m, state))
    for a, b in zip(res["rewards"], host["rewards"]):
        assert all(isinstance(x, float) for x in a)
        np.testing.assert_allclose(a, b, atol=1e-5)
    table = result.table()
    np.testing.assert_equal(table, ev.summarize(res))    # (exact; NaN == NaN: the Va rise time of these five is undefined)
    assert set(table) == set(ev.summarize(host)) and all(set(table[k]) == set(v) for k, v in ev.summarize(host).items())
    assert np.isnan(result.rewards[result.length[0]:, 0]).all() and not np.isnan(result.rewards[:result.length[0], 0]).any()


def test_missing_pid_column_raises_like_the_host_loop():
    cfg = configs.reference_like("examples")
    cfg["observation"]["states"] = [s for s in cfg["observation"]["states"] if s["name"] != "omega_q"]
    with pytest.raises(ValueError, match="When using PID roll, pitch, Va, omega_p, omega_q, omega_r must be part"):
        ev.evaluate_on_set_device(_scenarios()[:2], cfg, _backend=HostBackend(), _lib_path=build_emu())


class _CountingBackend(HostBackend):
    def __init__(self):
        self.reads = 0

    def to_host(self, t):
        self.reads += 1
        return HostBackend.to_host(self, t)

    def sync(self):
        self.reads += 1


def test_no_host_traffic_inside_a_chunk():
    from gym_fixed_wing.pid import DevicePID
    from gym_fixed_wing.vec_env import FixedWingVecEnv
    scen, mem, chunk = _scenarios()[:5], _CountingBackend(), 50
    vec = FixedWingVecEnv(configs.reference_like("examples"), num_envs=len(scen), config_kw=ev.evaluation_overrides(True),
                          sim_config_kw={"turbulence": False, "turbulence_intensity": "none"}, auto_reset=False, _backend=mem,
                          _lib_path=build_emu())
    run = ev.DeviceEvaluation(vec, DevicePID(vec))
    run.reset(scen)
    before = mem.reads
    steps = run.run(chunk)
    during = mem.reads - before
    vec.close()
    assert steps >= 100 and steps % chunk == 0
    assert during <= edc.ceil_div(steps, chunk) + 2, (during, steps)
    assert during >= 1
