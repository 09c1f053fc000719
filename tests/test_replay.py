"""The device hindsight replay buffer (include/fwgym.h "Hindsight replay", gym_fixed_wing.replay) on the HOST EMULATION of the
kernels -- the CPU half; tests/test_replay_gpu.py is the GPU half and shares the bodies (tests/replay_common.py).

  exports      fwg_replay_index / fwg_replay_sample, the Philox stream, the ABI version (still 26);
  index        fwg_replay_index against a numpy backward scan, every done pattern, T x N = 140 x 130 and 1 x 1, guard row;
  sample       fwg_replay_sample against the numpy restatement: three configurations (a delta factor, the potential form, no delta
               factor) x D 14 / 60 x n_filled 1 / 3 x three strategies x p 0 / 2^31 / 2^32, 4096 samples each -- index exact, gathered
               rows bit-equal, rewards of relabelled samples within gc.REWARD_TOL, guard rows, no empty class;
  determinism  the same (seed, serial) twice, another serial;
  layer        HindsightReplay: four rollouts into three slots beside a twin without a replay, sample() against the restatement;
  refusals     status codes and messages, nothing launched; ValueErrors of the Python layer;
  resources    the committed report lists the two kernels: no scratch frame, no spills."""
import os

import pytest

import goal_common as gc
import replay_common as rc
from emu.host_backend import HERE as EMU_HERE, HostBackend, build_emu as _build_emu
from gym_fixed_wing import _native as nat

# tools/mutation_check.py re-runs this file against kernel sources with a bug put in (the replay_* mutants)
MUT_SRC, MUT_TAG = os.environ.get("FWGYM_MUTANT_SRC"), os.environ.get("FWGYM_MUTANT_TAG", "")


def build_emu():
    return _build_emu(src=MUT_SRC, out=os.path.join(EMU_HERE, "libfwgym_emu{}.so".format(MUT_TAG))) if MUT_SRC else _build_emu()


@pytest.fixture(scope="module")
def kw():
    return {"_backend": HostBackend(), "_lib_path": build_emu()}


def test_the_library_exports_the_replay_calls(kw):
    lib = nat.load_library(kw.get("_lib_path"))
    assert {"fwg_replay_index", "fwg_replay_sample"} <= set(nat.PROTOTYPES)
    assert hasattr(lib, "fwg_replay_index") and hasattr(lib, "fwg_replay_sample")
    assert nat.STREAM_REPLAY == 11 and nat.REPLAY_STRATEGIES == {"future": 0, "final": 1, "episode": 2}
    assert lib.fwg_abi_version() == nat.FWG_ABI_VERSION == 26


@pytest.mark.parametrize("t,n", [(rc.T_BIG, rc.N_BIG), (1, 1)])
def test_replay_index_is_the_backward_scan(kw, t, n):
    rc.index_case(kw, t, n)


@pytest.mark.parametrize("d", [14, 60])
@pytest.mark.parametrize("kind", rc.KINDS)
def test_replay_sample_matches_the_restatement(kw, kind, d):
    rc.sample_cells(kw, kind, d)


def test_replay_sample_is_a_function_of_seed_and_serial(kw):
    rc.determinism_case(kw)


def test_hindsight_replay_stores_rollouts_and_samples_them(kw):
    rc.python_layer(kw)


def test_replay_entry_points_refuse_what_they_cannot_serve(kw):
    res = rc.refusals(kw)
    assert len(res) == 28, sorted(res)
    assert "nothing is stored" in res["n_filled 0"] and "strategy" in res["unknown strategy"] and "240" in res["obs_words 241"]


def test_replay_kernels_use_no_scratch_and_spill_nothing():
    """The committed resource report of the product build (gym_fixed_wing/kernel_resources.json, whose source hash
    tests/test_kernel_resources.py pins) lists the replay kernels: no scratch frame, no spills."""
    import json
    from gym_fixed_wing import specialize
    with open(specialize.RESOURCES_JSON) as f:
        kernels = json.load(f)["kernels"]
    found = {n.split("(")[0]: r for n, r in kernels.items() if n.startswith("k_replay")}
    assert set(found) == {"k_replay_index", "k_replay_sample"}, sorted(found)
    for name, r in found.items():
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            assert r[key] == 0, (name, key, r[key])
