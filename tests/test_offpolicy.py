"""DDPG(update="hip"): the off-policy update as HIP kernels (include/fwgym.h "Off-policy update", gym_fixed_wing/offpolicy.py,
csrc/fwgym_offpolicy.h) -- both gradient launches against float64 autograd of ddpg_losses, the TD target alone, Adam and the Polyak
pass against torch.optim.Adam and lerp_, whole updates against the torch path, bitwise determinism, the real replay buffer in front of
it, the refusals and the kernels' resources; on the host emulation (CPU) and on the GPU.  The bodies and the reasoning behind the inputs
and the bounds: tests/offpolicy_common.py."""
import json
import os

import pytest
import torch

import offpolicy_common as oc
from gym_fixed_wing import _native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _emu():
    from emu.host_backend import build_emu
    return nat.load_library(build_emu()), "cpu"


def _gpu():
    return nat.load_library(), torch.device("cuda", 0)


def test_the_library_exports_the_offpolicy_calls():
    lib, _ = _emu()
    for name in ("fwg_offpolicy_create", "fwg_offpolicy_destroy", "fwg_offpolicy_num_params", "fwg_ddpg_critic_grad", "fwg_ddpg_actor_grad",
                 "fwg_ddpg_apply", "fwg_ddpg_step"):
        assert hasattr(lib, name) and name in nat.PROTOTYPES
    with open(os.path.join(ROOT, "include", "fwgym.h")) as f:
        header = f.read()
    assert "Off-policy update" in header and "fwg_offpolicy_batch" in header and "fwg_ddpg_hparams" in header


@pytest.mark.parametrize("shape", oc.SHAPES)
@pytest.mark.parametrize("NC", [1, 2])
def test_the_rejection_loop_terminates_and_keeps_most_rows(shape, NC):
    """At most half of the rows are rejected per pass (the weights are scaled for it, not the threshold), for every shape."""
    D, G, A = shape
    counts = []
    nets = oc.make_nets(D, G, A, NC, 31)
    b = oc.make_batch(nets, 1024, 32, counts=counts)
    print(shape, NC, counts)
    assert counts[0][0] == 1024 and counts[0][1] <= 512 and len(counts) <= 12
    assert 0.15 <= float(b["done"].float().mean()) <= 0.35
    with torch.no_grad():   # tanh neither linear nor saturated
        pi = nets[0](b["observation"], b["desired_rows"][:, :G]).abs()
    assert 0.2 <= float(pi.mean()) <= 0.9, float(pi.mean())


@pytest.mark.parametrize("shape", oc.SHAPES)
@pytest.mark.parametrize("B", [1, 65, 257])
@pytest.mark.parametrize("NC", [1, 2])
def test_gradients_match_float64_autograd_emulated(B, shape, NC):
    lib, dev = _emu()
    oc.check_grads(lib, dev, B, shape, NC, 7 + B + shape[0])


@pytest.mark.parametrize("B,shape,NC", [(1, (11, 3, 3), 1), (65, (11, 3, 3), 2), (257, (57, 3, 4), 2)])
def test_td_target_is_the_reward_on_terminal_rows_and_at_gamma_zero_emulated(B, shape, NC):
    lib, dev = _emu()
    oc.check_td_target(lib, dev, B, shape, NC, 17 + B)


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
def test_apply_matches_adam_and_lerp_emulated(max_grad_norm):
    lib, dev = _emu()
    oc.check_apply(lib, dev, max_grad_norm)


def test_hip_updates_match_the_torch_updates_emulated():
    lib, dev = _emu()
    oc.check_updates(lib, dev, oc.fixed_batches((11, 3, 3), 1, 257), (11, 3, 3))


def test_hip_updates_match_the_torch_updates_twin_delayed_emulated():
    lib, dev = _emu()
    oc.check_updates(lib, dev, oc.fixed_batches((11, 3, 3), 2, 257), (11, 3, 3), n_critics=2, policy_delay=2)


def test_hip_updates_match_the_torch_updates_clipped_emulated():
    """Both paths with max_grad_norm=0.05, below the gradients' norms: clip_grad_norm_ per segment, the twin critics under one norm."""
    lib, dev = _emu()
    oc.check_updates(lib, dev, oc.fixed_batches((11, 3, 3), 2, 257), (11, 3, 3), n_critics=2, max_grad_norm=0.05)


def test_end_to_end_with_the_replay_buffer_emulated():
    from emu.host_backend import HostBackend, build_emu
    lib, dev = _emu()
    oc.check_end_to_end(lib, dev, {"_backend": HostBackend(), "_lib_path": build_emu()}, 70, 300)


def test_refusals_name_their_argument_emulated():
    lib, dev = _emu()
    oc.check_refusals(lib, dev)


def test_save_load_and_act_emulated(tmp_path):
    lib, dev = _emu()
    oc.check_save_load(lib, dev, tmp_path)


def test_the_ddpg_kernels_fit_their_registers():
    """From the build's own report: no k_ddpg_ kernel has a scratch frame or spills a vector register, and none needs more than the
    512 registers of a lane."""
    with open(os.path.join(ROOT, "fixed-wing-gym_amd", "gym_fixed_wing", "kernel_resources.json")) as f:
        rep = json.load(f)
    kernels = {k.split("(")[0]: v for k, v in rep["kernels"].items() if k.startswith("k_ddpg_")}
    assert set(kernels) == {"k_ddpg_critic_grad", "k_ddpg_actor_grad", "k_ddpg_reduce", "k_ddpg_apply", "k_ddpg_polyak"}, sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512, (name, r)


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", oc.SHAPES)
@pytest.mark.parametrize("B", [1, 65, 257, 4096, 65536])
@pytest.mark.parametrize("NC", [1, 2])
def test_gradients_match_float64_autograd_on_gpu(B, shape, NC):
    lib, dev = _gpu()
    oc.check_grads(lib, dev, B, shape, NC, 7 + (B % 1000) + shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize("B,shape,NC", [(65, (11, 3, 3), 2), (4096, (57, 3, 4), 2)])
def test_td_target_is_the_reward_on_terminal_rows_and_at_gamma_zero_on_gpu(B, shape, NC):
    lib, dev = _gpu()
    oc.check_td_target(lib, dev, B, shape, NC, 17 + B)


@pytest.mark.gpu
@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
def test_apply_matches_adam_and_lerp_on_gpu(max_grad_norm):
    lib, dev = _gpu()
    oc.check_apply(lib, dev, max_grad_norm)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"n_critics": 2, "policy_delay": 2}, {"n_critics": 2, "max_grad_norm": 0.05}])
def test_hip_updates_match_the_torch_updates_on_gpu(kw):
    lib, dev = _gpu()
    oc.check_updates(lib, dev, oc.fixed_batches((11, 3, 3), kw.get("n_critics", 1), 4096), (11, 3, 3), **kw)


@pytest.mark.gpu
def test_end_to_end_with_the_replay_buffer_on_gpu():
    """(specialize=False: 1 024 envs x 32 steps on the generic step kernel -- what is under test is the learner behind the buffer)"""
    import warnings
    lib, dev = _gpu()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        oc.check_end_to_end(lib, dev, {"device": 0, "specialize": False}, 1024, 4096)


@pytest.mark.gpu
def test_the_her_example_trains_with_the_hip_update():
    """examples/train_her.py --update hip --twin --policy-delay 2 for two iterations in a fresh child process: finite losses."""
    import subprocess
    import sys
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_her.py"), "--envs", "64", "--iters", "2", "--n-steps", "8", "--batch", "256",
           "--update", "hip", "--twin", "--policy-delay", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("iter")]
    assert len(lines) == 2, r.stdout
    for l in lines:
        words = l.replace("=", " ").split()
        losses = [float(words[words.index(k) + 1]) for k in ("critic_loss", "actor_loss")]
        assert np.isfinite(losses).all() and losses[0] > 0.0, l


@pytest.mark.gpu
def test_refusals_name_their_argument_on_gpu():
    lib, dev = _gpu()
    oc.check_refusals(lib, dev)


@pytest.mark.gpu
def test_save_load_and_act_on_gpu(tmp_path):
    lib, dev = _gpu()
    oc.check_save_load(lib, dev, tmp_path)
