"""The CNN rollout head (fwgym_actor.h: k_actor_act_cnn<SPLIT> = actor_block<SPLIT, 3, true>; the paper's controller, what
examples/train_ppo.py --policy cnn and the device evaluation run) against float64 over its shape contract, on the helpers of
tests/test_actor_contract.py.  What the CNN branch has of its own, and what pins it here:

  * the window load (15 float4s per lane through actor_obs_at; on a row log every row on its own plane), the normalisation and
    clip of the `xn[...]` line, the norm_obs store split between the two halves of a tile, the conv on the VALU (36 outputs, 5
    FMAs each, a bias per filter, tanhf), the k-slot map (36 outputs in three k-blocks of 16, 12 padded slots), and the two kernel
    instances (split-bf16 products and single products);
  * a. the forward pass per element over batches with a tile edge (1 / 31 / 32 / 33 / 255 / 256 / 257 / 513 envs), act_dim 1..4,
    training statistics, guard rows behind every buffer;  b. the single-product instance;  c. the row log read in place across
    wraps of the window position and episode ends, against float64 on the dense observation and bit for bit against a second head
    fed the dense batch;  d. non-default clip / epsilon / gamma with a third of the entries at the clip;  e. the sampling stream;
    f. MLP -> CNN -> MLP on one handle;  g. (GPU) a captured pair of acts and a captured rollout on the row log and on the dense env.

The yardstick is float64 numpy: _VecNorm64's statistics, the conv with tanh and the feature-major flatten (k = j * 3 + c) written
out below (_conv64; cross-checked against test_cnn_policy.np_forward), the two 64-64 tanh networks (_mlp64).  The error of an output
x against its reference is |x - ref| / max(|ref|, 1), per element (_err) -- never relative to the batch's largest output.
tools/mutation_check.py re-runs the emulated forms against kernel sources with a CNN head bug put back (head_cnn_*)."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import configs
from gym_fixed_wing.actor import DeviceActor, load_controller, weights_from_module
from gym_fixed_wing.rollout import CnnMlpPolicy
from gym_fixed_wing.vec_env import FixedWingVecEnv
from oracle import physics as oph
from test_actor_contract import (F32, LOG_2PI_HALF, OBS_TOL, PLAIN_TOL, STREAM_POLICY, _batch, _check_captured_pair, _check_stats,
                                 _emu, _err, _gpu, _Head, _mlp64, _obs_tol, _rewards, _var_atol_one_row, _VecNorm64, _weights)
from test_cnn_policy import np_forward

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, COLS, FILTERS = 5, 12, 3
D = ROWS * COLS   # the head's window: fwg_actor_set_conv refuses any other

# ---- bounds ----------------------------------------------------------------------------------------------------------------------
# mean and value of the split-bf16 instance, by the rule of tests/test_actor_contract.py: 2 x the worst error measured against the
# float64 reference over the cases of this file (profiles/actor_contract_errors.txt, the CNN tables), never above 1e-4; the margin
# is for other data seeds and box-to-box accumulation order.  Worst on the kernel's own normalised observation: 3.07e-5 on the
# MI355X (the row log, n 257, mean), 2.59e-5 on the host emulation (the row log, n 33, value); end to end 3.12e-5 on the MI355X (the
# same run) and 2.57e-5 on the emulation.  The conv adds nothing to the MLP head's figures (3.66e-5 / 3.42e-5 there): fp32 FMAs and
# tanhf in front of the same three k-blocks.
CNN_TOL_ISO = 6.2e-5   # against the float64 conv + networks on the kernel's own normalised observation
CNN_TOL_E2E = 6.3e-5   # against float64 from the raw observation
assert CNN_TOL_ISO <= 1e-4 and CNN_TOL_E2E <= 1e-4


# ---- weights and the float64 yardstick -------------------------------------------------------------------------------------------
def _weights_cnn(A, seed):
    """CnnMlpPolicy(act_dim=A): conv weights N(0, 0.8), three distinct non-zero conv biases, linear weights x 2.5 (tanh leaves its
    linear range), non-zero linear biases -> dict of float32 arrays (torch layout)."""
    torch.manual_seed(seed)
    pol = CnnMlpPolicy(act_dim=A)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        pol.conv.weight.copy_(0.8 * torch.randn(pol.conv.weight.shape, generator=g))
        pol.conv.bias.copy_(torch.tensor([0.35, -0.2, 0.6]))
        pol.log_std.copy_(torch.tensor([-0.3, 0.1, 0.4, -0.6][:A]))
        for net in (pol.pi, pol.vf):
            for m in net:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(2.5)
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    w = weights_from_module(pol)
    assert len(set(w["c1_b"].tolist())) == FILTERS and np.all(w["c1_b"] != 0) and w["pi_w0"].shape == (64, COLS * FILTERS)
    return w


def _conv64(w, x):
    """The conv front end in float64, written out: x [n][60] (row r, feature j at 12 r + j) -> [n][36], input k = 3 j + c of the
    networks = tanh(b[c] + sum_r w[r][c] x[r][j])."""
    cw, cb = np.asarray(w["c1_w"], np.float64), np.asarray(w["c1_b"], np.float64)
    x = np.asarray(x, np.float64)
    feat = np.empty((x.shape[0], COLS * FILTERS))
    for j in range(COLS):
        for c in range(FILTERS):
            z = np.full(x.shape[0], cb[c])
            for r in range(ROWS):
                z = z + cw[r, c] * x[:, COLS * r + j]
            feat[:, FILTERS * j + c] = np.tanh(z)
    return feat


def _cnn64(w, x):
    """-> (mean [n][A], value [n]) of the float64 policy on the normalised observations x [n][60]."""
    feat = _conv64(w, x)
    return _mlp64(w, "pi", feat), _mlp64(w, "vf", feat)[:, 0]


def test_the_float64_conv_written_here_equals_np_forward():
    w = _weights_cnn(4, 7)
    x = np.clip(np.random.default_rng(7).normal(size=(37, D)) * 3, -10, 10)
    mean, val = _cnn64(w, x)
    m2, v2 = np_forward(w, x, "tanh", "nhwc")
    np.testing.assert_allclose(mean, m2, rtol=0, atol=1e-13)
    np.testing.assert_allclose(val, v2, rtol=0, atol=1e-13)
    assert np.abs(mean).max() > 0.1


def _score(worst, w, out, want_no):
    """Mean and value of `out` against float64 on the kernel's own normalised observation (iso) and on `want_no` (e2e), folded
    into `worst`.  -> (iso, e2e) references"""
    iso, e2e = _cnn64(w, out["norm_obs"].astype(np.float64)), _cnn64(w, want_no)
    for key, got, a, b in (("mean", out["action"], iso[0], e2e[0]), ("value", out["value"], iso[1], e2e[1])):
        worst[key + "_iso"] = max(worst.get(key + "_iso", 0.0), _err(got, a))
        worst[key + "_e2e"] = max(worst.get(key + "_e2e", 0.0), _err(got, b))
    return iso, e2e


def _rew_tol(ref, rew):
    """The bound on the normalised reward under the statistics of `ref`: OBS_TOL, and for ONE-row batches what their conditioning
    adds, as _obs_tol does for the observation.  There every batch of returns has variance 0 and the running variance starts near
    1e-4 (count 1e-4, one row): it is off by up to _var_atol_one_row (the fixed-point quantum of the batch sums), which moves
    1 / std by |normalised reward| / (2 var) of it."""
    if ref.ret.shape[0] > 1:
        return OBS_TOL
    return OBS_TOL + 0.5 * np.abs(ref.raw_rew(rew)) * _var_atol_one_row(ref.dmax_ret) / (ref.ret_rms.var + ref.eps)


def _fmt(worst):
    return " ".join("{}={:.3g}".format(k, v) for k, v in worst.items())


def _assert_split_bounds(worst):
    assert worst["mean_iso"] <= CNN_TOL_ISO and worst["value_iso"] <= CNN_TOL_ISO, worst
    assert worst["mean_e2e"] <= CNN_TOL_E2E and worst["value_e2e"] <= CNN_TOL_E2E, worst


# ---- a. the forward pass over the shape contract ---------------------------------------------------------------------------------
def _run_forward(lib, mem, n, A, precise=True, steps=3):
    """Three observe / act steps (training statistics, deterministic; rewards and dones from the second on).  -> the worst errors
    and the last step's (mean, value) with their two float64 references."""
    seed = 1000 * D + 10 * A + n
    w = _weights_cnn(A, seed)
    rng = np.random.default_rng(seed)
    head = _Head(lib, mem, n, D, A, w, precise=precise, seed=11, env_id_base=5)
    assert head.actor.cnn
    ref = _VecNorm64(n, D)
    scale, shift = rng.uniform(0.5, 4.0, D).astype(F32), rng.uniform(-5, 5, D).astype(F32)
    worst = {k: 0.0 for k in ("obs", "obs_of_tol", "rew", "rew_of_tol", "mean_iso", "value_iso", "mean_e2e", "value_e2e")}
    logp_det = float(-(np.asarray(w["log_std"], np.float64) + LOG_2PI_HALF).sum())
    last = None
    for t in range(steps):
        obs = (rng.normal(size=(n, D)).astype(F32) * scale + shift)
        rew = done = None
        if t > 0:
            rew = (rng.normal(size=n) * 3 - 1).astype(F32)
            done = (rng.uniform(size=n) < 0.2).astype(np.uint8)
        out = head.step(obs, rew, done, deterministic=True)
        ref.observe(obs, rew, done)
        ref.fold()
        w_no = ref.norm_obs(obs)
        e_obs = np.abs(out["norm_obs"] - w_no)
        worst["obs"] = max(worst["obs"], float(e_obs.max()))
        worst["obs_of_tol"] = max(worst["obs_of_tol"], float(np.max(e_obs / _obs_tol(ref, obs))))
        iso, e2e = _score(worst, w, out, w_no)
        np.testing.assert_allclose(out["logp"], np.full(n, logp_det), rtol=1e-5)
        if rew is not None:
            e_rew = np.abs(out["norm_reward"] - ref.norm_rew(rew))
            worst["rew"] = max(worst["rew"], float(e_rew.max()))
            worst["rew_of_tol"] = max(worst["rew_of_tol"], float(np.max(e_rew / _rew_tol(ref, rew))))
            np.testing.assert_array_equal(out["done_out"], done)
        last = (out["action"], out["value"], iso, e2e)
    worst["obs_var"], worst["ret_var"] = _check_stats(head, ref, "cnn forward")
    head.close()
    return worst, last


def _check_forward_case(lib, mem, where, n, A):
    worst, _ = _run_forward(lib, mem, n, A)
    print("ACTOR_CONTRACT cnn forward {} n={} A={}: ".format(where, n, A) + _fmt(worst))
    assert worst["obs_of_tol"] <= 1.0 and worst["rew_of_tol"] <= 1.0, worst   # (the largest error / _obs_tol, / _rew_tol)
    _assert_split_bounds(worst)


# (n, A), pairwise: n = one env, a wave tile and a workgroup -1 / 0 / +1, two workgroups and a tail; A in 1..4
GPU_FWD_CASES = [(1, 4), (31, 1), (32, 3), (33, 2), (255, 4), (256, 2), (257, 1), (513, 3)]
EMU_FWD_CASES = [(1, 4), (33, 2), (65, 3), (257, 1)]


def _ids(cases):
    return ["n{}-A{}".format(*c) for c in cases]


@pytest.mark.parametrize("n,A", EMU_FWD_CASES, ids=_ids(EMU_FWD_CASES))
def test_forward_over_the_shape_contract_emulated(n, A):
    lib, mem = _emu()
    _check_forward_case(lib, mem, "emu", n, A)


@pytest.mark.gpu
@pytest.mark.parametrize("n,A", GPU_FWD_CASES, ids=_ids(GPU_FWD_CASES))
def test_forward_over_the_shape_contract_on_gpu(n, A):
    lib, mem = _gpu()
    _check_forward_case(lib, mem, "gpu", n, A)


# ---- b. single products (k_actor_act_cnn<1>) -------------------------------------------------------------------------------------
def _check_plain_mode(lib, mem, where, n, A):
    """precise=False: close to float64 in test_actor.py's measure (relative to the largest output of the batch), and really another
    arithmetic than the split instance, which meets its own bound on the same data."""
    (_, (mean1, val1, iso1, _)), (ws, (mean3, val3, _, _)) = (_run_forward(lib, mem, n, A, precise=p) for p in (False, True))
    rel = lambda x, r: float(np.abs(x - r).max() / np.abs(r).max())
    e_mean, e_val, diff = rel(mean1, iso1[0]), rel(val1, iso1[1]), rel(mean1, mean3)
    print("ACTOR_CONTRACT cnn plain {} n={} A={}: mean={:.3g} value={:.3g} against_split={:.3g} split: {}".format(where, n, A, e_mean, e_val, diff, _fmt(ws)))
    assert e_mean < PLAIN_TOL and e_val < PLAIN_TOL, (e_mean, e_val)
    assert diff > 1e-5, diff
    _assert_split_bounds(ws)


PLAIN_CASES = [(65, 3), (33, 2)]


@pytest.mark.parametrize("n,A", PLAIN_CASES, ids=_ids(PLAIN_CASES))
def test_single_product_instance_emulated(n, A):
    lib, mem = _emu()
    _check_plain_mode(lib, mem, "emu", n, A)


@pytest.mark.gpu
@pytest.mark.parametrize("n,A", PLAIN_CASES, ids=_ids(PLAIN_CASES))
def test_single_product_instance_on_gpu(n, A):
    lib, mem = _gpu()
    _check_plain_mode(lib, mem, "gpu", n, A)


# ---- c. the row log read in place, across wraps of the window position and episode ends ------------------------------------------
class _LogHead(_Head):
    """A _Head whose inputs are the env's own buffers (the row log, the step's rewards and flags), read in place; the outputs stay
    guarded."""

    def _inputs(self, obs, rew, done):
        return (obs, rew, done), (obs, rew, done)


def _check_row_log(where, vec, steps, seed):
    """`steps` env steps under random actions; after each a training head on the row log observes and acts.  Every act: the
    normalised observation, mean and value against float64 on the dense observation the env returns, and every output bit for bit
    against a second head fed that dense batch.  The statistics start from the shipped controller's (tests/golden/cnn_controller.npz)
    with count n, so every fold still moves them.  From RunningMeanStd's own start (mean 0, var 1, count 1e-4) the first folds of a
    few just-reset envs are outside what OBS_TOL was set for, for two reasons that are the fold's and not the window read's: the
    first batch lies 30 standard deviations from the running mean (the fp32 cancellation of _var_rtol: measured 2e-4 of the
    variance, 1.9e-4 of a normalised entry), and some features vary by 4e-3 over 33 just-reset envs, a variance of 1.5e-5 against
    the batch sums' fixed-point quantum 2^-20 / n (measured 4.8e-4 of the variance, 5.7e-5 of an entry)."""
    lib, mem, n, A = vec._lib, vec._mem, vec.num_envs, 3
    assert vec.obs_log_rows > 0 and vec.obs_shape == (ROWS, COLS) and int(vec._c.obs_step) == 2
    L, S, period = vec.obs_log_rows, int(vec._c.obs_step), vec.obs_window_period
    w = _weights_cnn(A, seed)
    log, dense = _LogHead(lib, mem, n, D, A, w, seed=11, env_id_base=5), _Head(lib, mem, n, D, A, w, seed=11, env_id_base=5)
    log.actor.set_obs_log(vec)
    ref = _VecNorm64(n, D)
    rng = np.random.default_rng(seed)
    vec.reset()
    shipped = load_controller(os.path.join(HERE, "golden", "cnn_controller.npz"))["obs_rms"]
    given = (np.asarray(shipped["mean"]).reshape(-1), np.asarray(shipped["var"]).reshape(-1), float(n))
    for s in (log.actor, dense.actor, ref):
        s.set_stats(*given)
    worst = {"obs": 0.0, "obs_of_tol": 0.0}
    wraps, ends, after_wrap, after_reset, last_pos = [0] * S, 0, 0, 0, {}
    for t in range(steps):
        o, r, d = vec.step_device(mem.from_host(rng.uniform(-1, 1, size=(n, 3)).astype(F32)))
        mem.sync()
        obs = np.ascontiguousarray(mem.to_host(o)).reshape(n, D).copy()
        rew, done = np.array(mem.to_host(r)), np.array(mem.to_host(d))
        plane = ctypes.c_int64()
        assert lib.fwg_obs_window(vec._handle, ctypes.byref(plane)) == 0
        parity, pos = divmod(plane.value, L)
        wrapped = parity in last_pos and pos > last_pos[parity]   # (a parity's records descend; its wrap puts the window back on top)
        last_pos[parity] = pos
        wraps[parity] += wrapped
        after_wrap += wrapped
        ends += int(done.sum())
        after_reset += bool(done.any())
        a = log.step(vec._obs_buf, r, d)
        b = dense.step(obs, rew, done)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg="step {} {}: the head on the row log against the head on the dense batch".format(t, k))
        ref.observe(obs, rew, done)
        ref.fold()
        w_no = ref.norm_obs(obs)
        e_obs = np.abs(a["norm_obs"] - w_no)
        worst["obs"] = max(worst["obs"], float(e_obs.max()))
        worst["obs_of_tol"] = max(worst["obs_of_tol"], float(np.max(e_obs / _obs_tol(ref, obs))))
        _score(worst, w, a, w_no)
    print("ACTOR_CONTRACT cnn row_log {} n={} steps={} period={}: wraps per parity {} episode_ends={} acts_after_wrap={} acts_after_reset={} ".format(
        where, n, steps, period, wraps, ends, after_wrap, after_reset) + _fmt(worst))
    # what the run must have been for the comparison to mean something
    assert min(wraps) >= 2 and ends >= n and after_wrap >= 1 and after_reset >= 1, (wraps, ends, after_wrap, after_reset)
    assert worst["obs_of_tol"] <= 1.0, worst
    _assert_split_bounds(worst)
    log.close(), dense.close()


def test_row_log_across_wraps_and_episode_ends_emulated():
    from emu.host_backend import HostBackend
    lib, _ = _emu()
    vec = FixedWingVecEnv(configs.reference_like("cnn"), num_envs=33, config_kw={"observation": {"step": 2}, "steps_max": 9}, as_numpy=True,
                          _backend=HostBackend(), _lib_path=lib._name, obs_log_rows=10, seed=3)
    assert vec.obs_window_period == 12
    _check_row_log("emu", vec, 30, 71)
    vec.close()


@pytest.mark.gpu
def test_row_log_across_wraps_and_episode_ends_on_gpu():
    vec = FixedWingVecEnv(copy.deepcopy(configs.reference_like("cnn")), num_envs=257, device=0,
                          config_kw={"observation": {"step": 2}, "steps_max": 20}, seed=1)
    _check_row_log("gpu", vec, 2 * vec.obs_window_period + 10, 72)
    vec.close()


# ---- d. clipping and VecNormalize's arguments ------------------------------------------------------------------------------------
def _check_clipping(lib, mem, where):
    n, A = 100, 3
    rng = np.random.default_rng(2)
    kw = dict(gamma=0.9, clip_obs=2.5, clip_reward=1.5, epsilon=1e-2)
    w = _weights_cnn(A, 41)
    head = _Head(lib, mem, n, D, A, w, training=False, **kw)
    ref = _VecNorm64(n, D, 0.9, 2.5, 1.5, 1e-2, training=False)
    given = (rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D), 1000.0, 0.2, 1.7, 900.0)
    head.actor.set_stats(*given)
    ref.set_stats(*given)
    # inputs at 3 and 1.8 standard deviations of the statistics: P(|z| > 2.5 / 3) = P(|z| > 1.5 / 1.8) = 0.40 of them past the clip
    obs = (ref.obs_rms.mean + 3.0 * np.sqrt(ref.obs_rms.var) * rng.normal(size=(n, D))).astype(F32)
    rew = (1.8 * math.sqrt(ref.ret_rms.var) * rng.normal(size=n)).astype(F32)
    done = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    out = head.step(obs, rew, done)
    for key, got, raw, clip in (("obs", out["norm_obs"], ref.raw_obs(obs), 2.5), ("rew", out["norm_reward"], ref.raw_rew(rew), 1.5)):
        frac = float(np.mean(np.abs(raw) > clip))
        assert 0.25 <= frac <= 0.45, (key, frac)   # the reference itself reaches the clip
        want = np.clip(raw, -clip, clip)
        clipped = np.abs(raw) > clip + 1e-6      # (within 1e-6 of the clip fp32 and float64 may fall on either side)
        np.testing.assert_array_equal(got[clipped], want[clipped].astype(F32), err_msg=key + ": not exactly at the clip")
        assert np.abs(got - want).max() <= 1e-6, (key, float(np.abs(got - want).max()))
        assert np.abs(got).max() <= clip
    np.testing.assert_array_equal(out["done_out"], done)
    worst = {}
    _score(worst, w, out, ref.norm_obs(obs))
    print("ACTOR_CONTRACT cnn clipping {} n={} A={}: ".format(where, n, A) + _fmt(worst))
    _assert_split_bounds(worst)
    head.close()


def test_clipping_and_arguments_emulated():
    _check_clipping(*_emu(), "emu")


@pytest.mark.gpu
def test_clipping_and_arguments_on_gpu():
    _check_clipping(*_gpu(), "gpu")


# ---- e. sampling -----------------------------------------------------------------------------------------------------------------
def _check_sampling(lib, mem, A):
    """Deterministic and sampled acts alternating: the noise of act number c (every act counts) is the oracle's Philox stream 6 at
    (seed, env_id_base + env, c); a head whose env ids start one later draws the first head's rows 1.. as its rows 0.."""
    n = 33
    seed, base = (7 << 32) | 3, 1000
    w = _weights_cnn(A, 51)
    rng = np.random.default_rng(51)
    mean, var = rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D)
    head = _Head(lib, mem, n, D, A, w, training=False, seed=seed, env_id_base=base)
    other = _Head(lib, mem, n - 1, D, A, w, training=False, seed=seed, env_id_base=base + 1)
    for h in (head, other):
        h.actor.set_stats(mean, var, 1000.0)
    ls = np.asarray(w["log_std"], np.float64)
    sigma = np.exp(ls)
    counter = 0
    for rnd in range(3):
        obs = _batch(rng, n, D, 1.0, 0.0)
        det, det_o = head.step(obs, deterministic=True, observe=False), other.step(obs[1:], deterministic=True, observe=False)
        counter += 1
        smp, smp_o = head.step(obs, deterministic=False, observe=False), other.step(obs[1:], deterministic=False, observe=False)
        mu = det["action"].astype(np.float64)
        np.testing.assert_array_equal(smp["value"], det["value"])
        z = (smp["action"].astype(np.float64) - mu) / sigma
        want = oph.box_muller(oph.rng_bits(seed, base + np.arange(n), counter, STREAM_POLICY))[:, :A]
        counter += 1
        tol = 1e-5 * np.maximum(1.0, np.abs(mu) / sigma)   # (the action carries the mean: its fp32 rounding, in units of sigma)
        assert np.all(np.abs(z - want) <= tol), (rnd, float(np.max(np.abs(z - want) / tol)))
        logp = (-0.5 * want ** 2 - ls - LOG_2PI_HALF).sum(axis=1)
        np.testing.assert_allclose(smp["logp"], logp, rtol=1e-5)
        np.testing.assert_allclose(det["logp"], np.full(n, -(ls + LOG_2PI_HALF).sum()), rtol=1e-5)
        np.testing.assert_array_equal(det_o["action"], det["action"][1:])
        np.testing.assert_array_equal(smp_o["action"], smp["action"][1:])
        np.testing.assert_array_equal(smp_o["logp"], smp["logp"][1:])
    head.close(), other.close()


@pytest.mark.parametrize("A", [1, 4])
def test_sampling_noise_is_the_oracle_stream_emulated(A):
    _check_sampling(*_emu(), A)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 4])
def test_sampling_noise_is_the_oracle_stream_on_gpu(A):
    _check_sampling(*_gpu(), A)


# ---- f. MLP -> CNN -> MLP on one handle ------------------------------------------------------------------------------------------
def _check_policy_switch(lib, mem):
    """One DeviceActor(..., 60) loaded with an MLP policy (NK1 = 4), a CNN policy (NK1 = 3: fewer fragments, the conv parameters
    behind the biases), the MLP again: after each load every output equals that of a fresh head of that kind bit for bit -- no
    fragment, conv parameter or k-block count left over from the policy before."""
    n, A = 65, 3
    rng = np.random.default_rng(81)
    mean, var = rng.uniform(-1, 1, D), rng.uniform(0.5, 2, D)
    obs = _batch(rng, n, D, 1.5, 0.3)
    rew, done = _rewards(rng, n)
    for precise in (True, False):
        kw = dict(training=False, precise=precise, seed=4, env_id_base=2)
        policies = [("mlp", _weights(D, A, 82)), ("cnn", _weights_cnn(A, 83)), ("mlp", _weights(D, A, 82))]
        one = _Head(lib, mem, n, D, A, policies[0][1], **kw)
        one.actor.set_stats(mean, var, 1000.0)
        seen = {}
        for i, (kind, w) in enumerate(policies):
            one.actor.load_policy(w)
            assert one.actor.cnn == (kind == "cnn")
            fresh = _Head(lib, mem, n, D, A, w, **kw)
            fresh.actor.set_stats(mean, var, 1000.0)
            a, b = one.step(obs, rew, done, observe=False), fresh.step(obs, rew, done, observe=False)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg="load {} ({}, precise={}): {}".format(i, kind, precise, k))
            seen.setdefault(kind, a["action"])
            fresh.close()
        assert np.abs(seen["mlp"] - seen["cnn"]).max() > 1e-2   # (the two policies do differ on this batch)
        one.close()


def test_mlp_and_cnn_policies_on_one_handle_emulated():
    _check_policy_switch(*_emu())


@pytest.mark.gpu
def test_mlp_and_cnn_policies_on_one_handle_on_gpu():
    _check_policy_switch(*_gpu())


# ---- g. capture (GPU) ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_captured_pair_of_cnn_acts_equals_the_eager_sequence_on_gpu():
    lib, mem = _gpu()
    _check_captured_pair(lib, mem, 257, D, 2, _weights_cnn(2, 61), 61)


@pytest.mark.gpu
def test_graphed_cnn_rollout_on_row_log_env_matches_dense_over_replays_on_gpu(monkeypatch):
    """FusedRollout(graph=True) under a CNN head, on the row-log env and on the dense env: seven replays of a 10-step chunk, 70
    steps, past the 64-step period of the window position and past steps_max -- the head has to read the CURRENT window on every
    replay (the position is read on the device)."""
    from gym_fixed_wing.rollout import FusedRollout
    monkeypatch.setenv("FWGYM_SHAPE", "0")   # (both layouts on the same kernel tier: the dense one would land on a shape instance)
    cfg = configs.reference_like("cnn")
    turb = {"turbulence": True, "turbulence_intensity": "moderate"}
    n, runs = 512, []
    for rows in (0, None):   # dense, the default row log
        vec = FixedWingVecEnv(copy.deepcopy(cfg), num_envs=n, device=0, config_kw={"observation": {"step": 2}, "steps_max": 37},
                              sim_config_kw=copy.deepcopy(turb), obs_log_rows=rows, seed=4, derived_views=False)
        assert bool(vec.obs_log_rows) == (rows is None) and (rows == 0 or vec.obs_window_period == 64)
        vec.reset()
        actor = DeviceActor.for_env(vec, seed=5)
        actor.load_policy(_weights_cnn(3, 91))
        assert actor.cnn
        ro = FusedRollout(vec, actor, 10, graph=True)
        reps = []
        for rep in range(7):
            buf = ro.run()
            torch.cuda.synchronize()
            reps.append({k: v.detach().cpu().numpy().copy() for k, v in buf.items()})
        runs.append(reps)
        actor.close()
        vec.close()
    for rep, (a, b) in enumerate(zip(*runs)):
        for k in a:
            np.testing.assert_allclose(a[k], b[k], rtol=0, atol=2e-6, err_msg="replay {} {}".format(rep, k))
    ends = sum(int(r["dones"].sum()) for r in runs[0])
    print("ACTOR_CONTRACT cnn graphed_rollout gpu n={}: 7 replays x 10 steps, episode_ends={}".format(n, ends))
    assert ends >= n

