"""The behaviour head and the hindsight collector (include/fwgym.h "Behaviour head", gym_fixed_wing/behaviour.py,
csrc/fwgym_behaviour.h): the forward pass against float64, the exploration draws against a numpy restatement built on the oracle's
Philox, the goal rows against fwg_goal_observe, the collector against a loop of its parts and (GPU) against its own graph replay, the
refusals and the kernel's resources; on the host emulation (CPU) and on the GPU.  The bodies and the reasoning behind the bounds:
tests/behaviour_common.py."""
import json
import os

import pytest
import torch

import behaviour_common as bc
from gym_fixed_wing import _native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")


def _emu_path():
    from emu.host_backend import HERE as EMU, build_emu
    return build_emu(src=MUT_SRC, out=os.path.join(EMU, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else build_emu()


def _emu():
    return nat.load_library(_emu_path()), "cpu"


def _emu_env():
    from emu.host_backend import HostBackend
    return {"_backend": HostBackend(), "_lib_path": _emu_path()}


def _gpu():
    return nat.load_library(), torch.device("cuda", 0)


GPU_ENV = {"device": 0, "specialize": False}   # (the generic step kernel: what is under test is the head around it)


def _ids(shapes):
    return ["D{}-G{}-A{}".format(*s) for s in shapes]


def test_the_library_exports_the_behaviour_head():
    lib, _ = _emu()
    assert hasattr(lib, "fwg_behaviour_act") and "fwg_behaviour_act" in nat.PROTOTYPES
    with open(os.path.join(ROOT, "include", "fwgym.h")) as f:
        assert "Behaviour head" in f.read()
    assert lib.fwg_abi_version() == 26


# ---- 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bc.SHAPES, ids=_ids(bc.SHAPES))
@pytest.mark.parametrize("n", bc.BATCHES)
def test_forward_matches_float64_emulated(shape, n):
    bc.check_forward(*_emu(), shape, n)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", bc.SHAPES, ids=_ids(bc.SHAPES))
@pytest.mark.parametrize("n", bc.BATCHES)
def test_forward_matches_float64_on_gpu(shape, n):
    bc.check_forward(*_gpu(), shape, n)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------
def test_draws_are_exact_emulated():
    bc.check_draws(*_emu())


@pytest.mark.gpu
def test_draws_are_exact_on_gpu():
    bc.check_draws(*_gpu())


# ---- 3 -----------------------------------------------------------------------------------------------------------------------
def test_gaussian_noise_and_clipping_emulated():
    bc.check_gaussian_clipping(*_emu())


@pytest.mark.gpu
def test_gaussian_noise_and_clipping_on_gpu():
    bc.check_gaussian_clipping(*_gpu())


# ---- 4 -----------------------------------------------------------------------------------------------------------------------
def test_the_noise_stream_does_not_depend_on_the_batch_emulated():
    bc.check_stream_independence(*_emu())


@pytest.mark.gpu
def test_the_noise_stream_does_not_depend_on_the_batch_on_gpu():
    bc.check_stream_independence(*_gpu())


# ---- 5 -----------------------------------------------------------------------------------------------------------------------
def test_goal_rows_are_those_of_goal_observe_emulated():
    bc.check_goal_rows(*_emu(), _emu_env())


@pytest.mark.gpu
def test_goal_rows_are_those_of_goal_observe_on_gpu():
    bc.check_goal_rows(*_gpu(), GPU_ENV)


# ---- 6 -----------------------------------------------------------------------------------------------------------------------
def test_collector_equals_the_loop_of_its_parts_emulated():
    bc.check_collector(*_emu(), _emu_env())


@pytest.mark.gpu
def test_collector_equals_the_loop_of_its_parts_on_gpu():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        bc.check_collector(*_gpu(), GPU_ENV)


# ---- 7 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_equals_the_eager_collector_on_gpu():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        bc.check_graph_replay(*_gpu(), GPU_ENV)


# ---- 8 -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument_emulated():
    bc.check_refusals(*_emu(), _emu_env(), _emu_env())


@pytest.mark.gpu
def test_refusals_name_their_argument_on_gpu():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        bc.check_refusals(*_gpu(), GPU_ENV, GPU_ENV)


# ---- 9 -----------------------------------------------------------------------------------------------------------------------
def test_the_behaviour_kernel_fits_its_registers():
    """From the build's own report: k_behaviour_act has no scratch frame and spills no vector register."""
    with open(os.path.join(ROOT, "fixed-wing-gym_amd", "gym_fixed_wing", "kernel_resources.json")) as f:
        rep = json.load(f)
    kernels = {k.split("(")[0]: v for k, v in rep["kernels"].items() if k.startswith("k_behaviour_")}
    assert set(kernels) == {"k_behaviour_act"}, sorted(kernels)
    r = kernels["k_behaviour_act"]
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 512, r


# ---- 10 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_her_example_collects_on_the_device_under_a_graph():
    """examples/train_her.py --collect device --graph --update hip for two iterations in a fresh child process: finite losses."""
    import subprocess
    import sys
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train_her.py"), "--collect", "device", "--graph", "--update", "hip", "--envs", "1024",
           "--iters", "2", "--n-steps", "8", "--updates", "2", "--batch", "256"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("iter")]
    assert len(lines) == 2, r.stdout
    for l in lines:
        words = l.replace("=", " ").split()
        losses = [float(words[words.index(k) + 1]) for k in ("critic_loss", "actor_loss")]
        assert np.isfinite(losses).all() and losses[0] > 0.0, l
