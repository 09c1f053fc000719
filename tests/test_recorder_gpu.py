"""The device flight recorder, GPU half (the CPU half and the description of the shared bodies: tests/test_recorder.py,
tests/recorder_common.py).

  shared       every test of the CPU half, on the MI355X (same inputs, same restatement, same bound);
  graph replay two identically seeded envs with a recorder each, one under a replayed hipGraph (FusedRollout(graph=True)), one
               stepped eagerly: headers and rows bit-equal after every rollout, and the rollout buffers bit-equal to those of an
               env with no recorder (the recorder perturbs nothing) -- dense observations with an attached MLP head, the row log
               with the CNN head, and a hand-captured chunk of step_device calls whose length does not divide the episode length;
  refusals     attaching after a capture, the one-launch step with a recorder attached."""
import numpy as np
import pytest
import torch

import configs
import test_recorder as cpu_half
from gym_fixed_wing.actor import DeviceActor
from gym_fixed_wing.recorder import FlightRecorder
from gym_fixed_wing.rollout import CnnMlpPolicy, FusedRollout, MlpPolicy
from gym_fixed_wing.vec_env import FixedWingVecEnv

pytestmark = pytest.mark.gpu
GRAPH_N, GRAPH_TRACK, GRAPH_STEPS_MAX = 4096, (0, 64, 4095), 20


@pytest.fixture(scope="module")
def kw():
    return {"device": 0}


# the bodies of the CPU half take the backend through `kw`
test_kernels_match_the_numpy_restatement_bit_for_bit = cpu_half.test_kernels_match_the_numpy_restatement_bit_for_bit
test_entry_points_refuse_bad_arguments = cpu_half.test_entry_points_refuse_bad_arguments
test_recorded_episode_equals_the_single_env_history = cpu_half.test_recorded_episode_equals_the_single_env_history
test_an_abandoned_episode_is_never_completed = cpu_half.test_an_abandoned_episode_is_never_completed
test_a_failed_episode_has_no_terminal_state_row_as_in_the_single_env_class = \
    cpu_half.test_a_failed_episode_has_no_terminal_state_row_as_in_the_single_env_class
test_auto_reset_episodes_against_host_reads = cpu_half.test_auto_reset_episodes_against_host_reads
test_computed_derived_words_against_float64 = cpu_half.test_computed_derived_words_against_float64
test_render_and_env_method = cpu_half.test_render_and_env_method
test_no_render_before_the_first_episode_has_ended = cpu_half.test_no_render_before_the_first_episode_has_ended
test_constructor_refusals_and_detach = cpu_half.test_constructor_refusals_and_detach


# ------------------------------------------------------------------------------------------------------ 5. under graph replay
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


def _recorder_state(rec):
    return rec.hdr.cpu().numpy(), rec.rows.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("preset", ["examples", "cnn"])
def test_recorder_under_graph_replay_equals_eager_and_perturbs_nothing(preset):
    n_steps, replays = 8, 12
    runs = {}
    for name, graph, record in (("graph", True, True), ("eager", False, True), ("plain", True, False)):
        vec = _env(preset)
        assert bool(vec.obs_log_rows) == (preset == "cnn")
        vec.reset()
        rec = FlightRecorder(vec, env_ids=GRAPH_TRACK) if record else None
        vec.reset()                                      # (the recorder starts with a reset; the plain env resets twice as well)
        actor = _head(vec, preset)
        ro = FusedRollout(vec, actor, n_steps, graph=graph)
        assert not ro.fused
        if not graph:                                    # the two warm-up steps a capture takes before it records the graph
            ro._prime()
            ro._step(ro.cur["actions"], ro.cur)
            ro._step(ro.cur["actions"], ro.cur)
        runs[name] = (vec, rec, actor, ro)
    completed = 0
    for r in range(replays):
        bufs = {name: {k: v.cpu().numpy() for k, v in ro.run().items()} for name, (_, _, _, ro) in runs.items()}
        (h_g, r_g), (h_e, r_e) = _recorder_state(runs["graph"][1]), _recorder_state(runs["eager"][1])
        np.testing.assert_array_equal(h_g, h_e, err_msg="headers after rollout {}".format(r))
        np.testing.assert_array_equal(r_g, r_e, err_msg="rows after rollout {}".format(r))
        for k in bufs["graph"]:
            np.testing.assert_array_equal(bufs["graph"][k].view(np.uint8), bufs["plain"][k].view(np.uint8),
                                          err_msg="rollout {} buffer {}: recorder attached vs not".format(r, k))
            np.testing.assert_array_equal(bufs["graph"][k].view(np.uint8), bufs["eager"][k].view(np.uint8),
                                          err_msg="rollout {} buffer {}: graph vs eager".format(r, k))
        completed = int(h_g[:, 6].min())
    assert completed >= (2 + n_steps * replays) // GRAPH_STEPS_MAX - 1 and completed >= 3
    vec, rec = runs["graph"][:2]
    for k in range(len(GRAPH_TRACK)):
        ep = rec.episode(k, "last")
        assert ep.consistent and not ep.overflowed and 1 <= ep.length <= GRAPH_STEPS_MAX
        assert ep.episode_index + 1 == rec.episode(k, "current").episode_index
    for vec, _, actor, _ in runs.values():
        actor.close()
        vec.close()


def test_recorder_in_a_hand_captured_chunk_that_does_not_divide_the_episode():
    chunk, replays = 6, 9                                  # 6 does not divide 20: the episode ends wander through the chunk
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    actions = [(torch.rand((GRAPH_N, 3), device="cuda", generator=gen) * 2 - 1).contiguous() for _ in range(chunk)]
    envs = {}
    for name in ("graph", "eager"):
        vec = _env("examples")
        rec = FlightRecorder(vec, env_ids=GRAPH_TRACK)
        vec.reset()
        envs[name] = (vec, rec)
    vec, rec = envs["graph"]
    dev = vec._obs.device
    vec.set_graph_mode(True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                          # warm-up outside the capture
        vec.step_device(actions[0])
        vec.step_device(actions[1])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    token = vec.capture_begin(chunk)
    with torch.cuda.graph(graph):
        for t in range(chunk):
            vec.step_device(actions[t])
    vec.capture_end()
    with pytest.raises(RuntimeError, match="captured"):    # a recorder attached after the capture would never be replayed
        FlightRecorder(vec, env_ids=(1,))
    with pytest.raises(RuntimeError, match="captured"):    # and the graph holds this one's launches and buffers
        rec.detach()
    assert vec._recorder is rec
    e_vec, e_rec = envs["eager"]
    e_vec.step_device(actions[0])
    e_vec.step_device(actions[1])
    for r in range(replays):
        vec.replay_check(token)
        graph.replay()
        vec.note_replayed_steps(chunk)
        for t in range(chunk):
            e_vec.step_device(actions[t])
        (h_g, r_g), (h_e, r_e) = _recorder_state(rec), _recorder_state(e_rec)
        np.testing.assert_array_equal(h_g, h_e, err_msg="headers after replay {}".format(r))
        np.testing.assert_array_equal(r_g, r_e, err_msg="rows after replay {}".format(r))
    assert int(h_g[:, 6].min()) >= 2
    lengths = {rec.episode(k, "last").length for k in range(len(GRAPH_TRACK))}
    assert all(1 <= n <= GRAPH_STEPS_MAX for n in lengths)
    vec.close(), e_vec.close()


def test_the_one_launch_step_refuses_a_recorded_env():
    vec = FixedWingVecEnv(configs.reference_like("examples"), num_envs=GRAPH_N, device=0, derived_views=False, seed=2)
    vec.reset()
    actor = _head(vec, "examples")
    actor.attach(vec)
    assert actor.rollout_available(vec)
    rec = FlightRecorder(vec, env_ids=(0,))
    with pytest.raises(ValueError, match="two-launch"):
        FusedRollout(vec, actor, 4, fused=True)
    with pytest.raises(ValueError, match="two-launch"):
        actor.rollout_step(vec)
    assert not FusedRollout(vec, actor, 4, fused="auto").fused and not FusedRollout(vec, actor, 4).fused
    rec.detach()
    assert FusedRollout(vec, actor, 4, fused="auto").fused
    actor.close()
    vec.close()
