"""The off-policy update (csrc/fwgym_offpolicy.h, fwg_ddpg_*, gym_fixed_wing/offpolicy.py) against float64 over its whole shape
contract, so that a rewrite of the kernels for speed has to keep what they compute:

  1. both gradient launches and the four statistics for 16 (D, G, A) shapes -- critic widths 3 .. 64 on both sides of every
     16-column edge, goal widths 1 .. 4, 1 .. 4 actions -- at 1, 63, 64, 65 and 129 rows with one and two critics;
  2. every batch array behind NaN fences, `done` at an odd byte, the unused goal words NaN, y_out inside a sentinel buffer;
  3. 20 481 rows: 321 tiles split unevenly over the 256 workgroups, a one-row tail tile; then a small call on the same learner
     (stale slabs);
  4. k_ddpg_apply and k_ddpg_polyak against float64 clip + Adam and lerp with hyper-parameters no two of which are alike;
  5. fwg_ddpg_step equal to its halves bit for bit, with and without the delayed actor step;
  6. six updates checked half by half against float64 at the learner's own state;
  7. (GPU) a captured fwg_ddpg_step replayed on refilled buffers equal to eager steps.

The yardsticks are float64: autograd of ddpg_losses on float64 copies (computed on the fp32 data), clip + Adam and lerp written out
in tests/offpolicy_contract.py, where the bodies and the reasoning behind the inputs are.  Bounds: 1e-4 relative Frobenius error
per tensor, 1e-5 for statistics with offpolicy_common's scales, test_ppo_hip_contract._check_state's closeness for states.  The
emulated forms run on the host build of the kernels; tools/mutation_check.py re-runs them against kernel sources with a bug put in
(FWGYM_MUTANT_SRC / FWGYM_MUTANT_TAG)."""
import os

import pytest
import torch

import offpolicy_contract as ct
from gym_fixed_wing import _native as nat

MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")


def _emu():
    from emu.host_backend import HERE, build_emu
    path = build_emu(src=MUT_SRC, out=os.path.join(HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else build_emu()
    return nat.load_library(path), "cpu"


def _gpu():
    return nat.load_library(), torch.device("cuda", 0)


def _ids(shapes):
    return ["D{}-G{}-A{}".format(*s) for s in shapes]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ct.SHAPES, ids=_ids(ct.SHAPES))
@pytest.mark.parametrize("NC", [1, 2])
def test_every_case_finds_a_well_conditioned_seed_and_the_rejection_loop_holds(shape, NC):
    ct.check_seeds_and_rejection(shape, NC)


@pytest.mark.parametrize("shape", ct.SHAPES, ids=_ids(ct.SHAPES))
@pytest.mark.parametrize("B", ct.BATCHES)
@pytest.mark.parametrize("NC", [1, 2])
def test_gradients_over_the_shape_contract_emulated(shape, B, NC):
    lib, dev = _emu()
    ct.check_grads(lib, dev, shape, B, NC)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ct.SHAPES, ids=_ids(ct.SHAPES))
@pytest.mark.parametrize("B", ct.BATCHES)
@pytest.mark.parametrize("NC", [1, 2])
def test_gradients_over_the_shape_contract_on_gpu(shape, B, NC):
    lib, dev = _gpu()
    ct.check_grads(lib, dev, shape, B, NC)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ct.FENCED_SHAPES, ids=_ids(ct.FENCED_SHAPES))
@pytest.mark.parametrize("B", [1, 65])
def test_nothing_outside_the_batch_is_read_or_written_emulated(shape, B):
    lib, dev = _emu()
    ct.check_fenced(lib, dev, shape, B)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ct.FENCED_SHAPES, ids=_ids(ct.FENCED_SHAPES))
@pytest.mark.parametrize("B", [1, 65])
def test_nothing_outside_the_batch_is_read_or_written_on_gpu(shape, B):
    lib, dev = _gpu()
    ct.check_fenced(lib, dev, shape, B)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_uneven_tile_split_and_stale_slabs_emulated():
    """(about 30 s: 2 x 321 tiles on the host, the one emulated case above 256 tiles)"""
    lib, dev = _emu()
    ct.check_tile_split(lib, dev, (11, 3, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(11, 3, 3), (57, 3, 4)], ids=_ids([(11, 3, 3), (57, 3, 4)]))
def test_uneven_tile_split_and_stale_slabs_on_gpu(shape):
    lib, dev = _gpu()
    ct.check_tile_split(lib, dev, shape)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_apply_and_polyak_match_float64_emulated():
    lib, dev = _emu()
    ct.check_apply64(lib, dev)


@pytest.mark.gpu
def test_apply_and_polyak_match_float64_on_gpu():
    lib, dev = _gpu()
    ct.check_apply64(lib, dev)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_step_equals_its_halves_emulated():
    lib, dev = _emu()
    ct.check_step_equals_halves(lib, dev)


@pytest.mark.gpu
def test_step_equals_its_halves_on_gpu():
    lib, dev = _gpu()
    ct.check_step_equals_halves(lib, dev)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_a_whole_run_matches_float64_at_the_learners_own_state_emulated():
    lib, dev = _emu()
    ct.check_run64(lib, dev)


@pytest.mark.gpu
def test_a_whole_run_matches_float64_at_the_learners_own_state_on_gpu():
    lib, dev = _gpu()
    ct.check_run64(lib, dev)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_step_equals_the_eager_one_on_gpu():
    lib, dev = _gpu()
    ct.check_captured_equals_eager(lib, dev)
