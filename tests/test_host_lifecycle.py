"""The three create functions of the C ABI give everything back when one of their device allocations fails: FWG_ERR_HIP, the
caller's out-handle untouched, no allocation left alive.  CPU only, on the host emulation build, whose hipMalloc / hipFree count
the live allocations and can be told to fail the k-th next one (tests/emu/hip/hip_runtime.h)."""
import ctypes

import numpy as np
import pytest

import configs
from emu.host_backend import build_emu
from gym_fixed_wing import _native as nat
from gym_fixed_wing.config import EnvConfig

FWG_ERR_HIP = -3
SENTINEL = 0x5EED5EED


@pytest.fixture(scope="module")
def lib():
    lib = nat.load_library(build_emu())
    lib.emu_hip_live_allocations.restype, lib.emu_hip_live_allocations.argtypes = ctypes.c_long, []
    lib.emu_hip_fail_malloc.restype, lib.emu_hip_fail_malloc.argtypes = None, [ctypes.c_long]
    return lib


def _check_create(lib, create, destroy):
    """`create(out)` -> status, `destroy(handle)`: counts the K allocations of a create that succeeds, then fails each in turn."""
    base = lib.emu_hip_live_allocations()
    out = ctypes.c_void_p()
    assert create(out) == 0, lib.fwg_last_error()
    k_allocs = lib.emu_hip_live_allocations() - base
    destroy(out)
    assert lib.emu_hip_live_allocations() == base
    try:
        for k in range(1, k_allocs + 1):
            out = ctypes.c_void_p(SENTINEL)
            lib.emu_hip_fail_malloc(k)
            assert create(out) == FWG_ERR_HIP, k
            assert b"hipMalloc" in lib.fwg_last_error(), k
            assert out.value == SENTINEL, k
            assert lib.emu_hip_live_allocations() == base, k
    finally:
        lib.emu_hip_fail_malloc(0)
    return k_allocs


def test_env_create_frees_what_it_allocated(lib):
    n = 3
    cfg = EnvConfig(configs.reference_like("model_gaussian")).compile()   # simulator.model: the reset queues are allocated too
    lay = nat.Layout()
    nat.check(lib, lib.fwg_get_layout(ctypes.byref(cfg), ctypes.byref(lay)))
    arena = np.zeros(lay.rows * n, np.float32)
    k_allocs = _check_create(lib, lambda out: lib.fwg_create(ctypes.byref(cfg), n, 0, arena.ctypes.data, 0, ctypes.byref(out)),
                             lambda h: nat.check(lib, lib.fwg_destroy(h)))
    assert k_allocs == 6   # configuration x 2, success sums, NaN flag, ring positions, reset queues


@pytest.fixture
def head(lib):
    h = ctypes.c_void_p()
    nat.check(lib, lib.fwg_actor_create(0, 70, 12, 3, 0.99, 10.0, 10.0, 1e-8, ctypes.byref(h)))
    yield h
    lib.fwg_actor_destroy(h)


def test_actor_create_frees_what_it_allocated(lib):
    k_allocs = _check_create(lib, lambda out: lib.fwg_actor_create(0, 70, 12, 3, 0.99, 10.0, 10.0, 1e-8, ctypes.byref(out)),
                             lib.fwg_actor_destroy)
    assert k_allocs == 6   # statistics, moment accumulators, weights, biases, log_std, returns


def test_learner_create_frees_what_it_allocated(lib, head):
    k_allocs = _check_create(lib, lambda out: lib.fwg_learner_create(head, ctypes.byref(out)), lib.fwg_learner_destroy)
    assert k_allocs == 2   # partial-gradient slab, flat gradient
