"""Shared pieces of tests/test_replay.py (host emulation of the kernels) and tests/test_replay_gpu.py: the device hindsight replay
buffer (include/fwgym.h "Hindsight replay": fwg_replay_index, fwg_replay_sample; gym_fixed_wing.replay).  Every body runs through
either memory backend: `kw` are the FixedWingVecEnv keywords that select it.

ref_index / ref_sample restate the two calls in numpy from the header's definition, with tests/goal_common.py's philox4x32 and
RefReward (the float64 restatement of the reward function, itself pinned to the reference there).  Integer decisions and gathered
rows are compared bit for bit; the rewards of relabelled samples within gc.REWARD_TOL, the measured bound of the same device
function (goal_reward) -- no new number."""
import copy
import ctypes

import numpy as np

import goal_common as gc
from gym_fixed_wing import _native as nat
from gym_fixed_wing.goal import GoalLog, GoalSpec
from gym_fixed_wing.replay import HindsightReplay
from gym_fixed_wing.rollout import FusedRollout

NULL = ctypes.c_void_p()
SEED, SERIAL = 0x1234567890ABCDEF, 3
T_BIG, N_BIG, K_BIG, BATCH = 140, 130, 3, 4096
STRATEGIES = ("future", "final", "episode")
P_VALUES = (0, 1 << 31, 1 << 32)
KINDS = ("reward_mix", "default_potential", "default_no_delta")   # a delta factor (W = 5); the potential form; no delta factor
# the restated draw rule on the inputs of sample_cells("reward_mix", ...) at p_scaled 2^31, n_filled 3: samples per class
# (src >= 0, -1, -2, -3) and per slot
CLASS_COUNTS, SLOT_COUNTS = (1717, 1736, 593, 50), (1329, 1392, 1375)
FIELDS = ("obs", "actions", "raw", "dones", "ep_end", "ach", "des")


def replay_config(kind):
    if kind != "default_no_delta":
        return gc.goal_config(kind)
    cfg = gc.goal_config("default")
    cfg["reward"]["factors"] = [f for f in cfg["reward"]["factors"] if not (f["class"] == "action" and f.get("type") == "delta")]
    return cfg


# ------------------------------------------------------------------------------------------------- the numpy restatements
def ref_index(dones):
    """ep_end[t][n]: the first t_e > t with dones[t_e][n], or T -- a backward scan per column."""
    T, N = dones.shape
    out = np.empty((T, N), np.int32)
    nxt = np.full(N, T, np.int32)
    for t in range(T - 1, -1, -1):
        out[t] = nxt
        nxt = np.where(dones[t] != 0, t, nxt).astype(np.int32)
    return out


def mulhi(x, n):
    return ((np.asarray(x, np.uint64) * np.asarray(n, np.int64).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def ref_sample(ref, slots, n_filled, strategy, B, seed, serial, p_scaled, mode=1):
    """fwg_replay_sample restated (include/fwgym.h).  slots: {obs [K][T+1][N][D], actions [K][T][N][3], raw [K][T][N], dones, ep_end,
    ach / des [K][T+1][N][4]} host arrays.  -> {index int32 [B][4], observation, next_observation, action, achieved, desired (fp32, bit
    patterns to compare), reward float64 [B] (the raw reward's own float where src < 0), done, rel, s0, R}."""
    K, T, N = slots["dones"].shape
    W = ref.window
    i = np.arange(B, dtype=np.int64)
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    a = gc.philox4x32(i, serial, 0, nat.STREAM_REPLAY, lo, hi)
    b = gc.philox4x32(i, serial, 1, nat.STREAM_REPLAY, lo, hi)
    k, t, n = mulhi(a[0], n_filled), mulhi(a[1], T), mulhi(a[2], N)
    ach, des = slots["ach"], slots["des"]
    idx = (ach[k, t, n, 3].view(np.uint32) & 0xFFFF).astype(np.int64)
    R = slots["ep_end"][k, t, n].astype(np.int64)
    s0 = np.maximum(t - idx, 0)
    if strategy == "future":
        r = t + 1 + mulhi(b[0], R - t)
    elif strategy == "final":
        r = R.copy()
    else:
        r = s0 + 1 + mulhi(b[0], R - s0)
    src = np.where(a[3] >= np.uint64(p_scaled), -1, r)
    if ref.has_delta:
        src = np.where(np.minimum(idx, W - 1) > t, -3, src)
    done = slots["dones"][k, t, n]
    src = np.where(done != 0, -2, src).astype(np.int32)
    rel = src >= 0
    desired = des[k, t, n].copy()
    desired[:, 3] = 0
    achieved = ach[k, t + 1, n].copy()
    achieved[:, 3] = 0
    reward = slots["raw"][k, t, n].astype(np.float64)
    j = np.flatnonzero(rel)
    if len(j):
        kk, tt, nn = k[j], t[j], n[j]
        new = ach[kk, src[j], nn].copy()
        new[:, 3] = 0
        desired[j] = new
        win = np.zeros((W, len(j), 3), np.float32)
        for age in range(W):
            use = (age <= np.minimum(idx[j], W - 1)) & (tt - age >= 0)
            win[W - 1 - age] = np.where(use[:, None], slots["actions"][kk, np.maximum(tt - age, 0), nn], np.nan)   # (NaN: must not be read)
        reward[j] = ref(ach[kk, tt + 1, nn], new, ach[kk, tt, nn], win, idx[j], mode)
    return {"index": np.stack([k, t, n, src.astype(np.int64)], axis=1).astype(np.int32), "observation": slots["obs"][k, t, n],
            "next_observation": slots["obs"][k, t + 1, n], "action": slots["actions"][k, t, n], "achieved": achieved, "desired": desired,
            "reward": reward, "done": done, "rel": rel, "s0": s0, "R": R}


# ------------------------------------------------------------------------------------------------------ C calls on host arrays
def call_index(vec, dones):
    """fwg_replay_index on a host array -> int32 [T][N] (a guard row behind the output is checked)."""
    m_, lib = vec._mem, vec._lib
    T, N = dones.shape
    out = m_.from_host(np.full((T + 1, N), -777, np.int32), "i32")
    nat.check(lib, lib.fwg_replay_index(T, N, m_.ptr(m_.from_host(np.ascontiguousarray(dones, np.uint8), "u8")), m_.ptr(out), m_.stream()))
    got = gc.host(vec, out)
    assert (got[T] == -777).all(), "fwg_replay_index wrote past row T - 1"
    return got[:T]


class DeviceSlots(object):
    """Host slot arrays uploaded once, and the fwg_replay_view over them."""

    def __init__(self, vec, slots):
        m_ = vec._mem
        kinds = {"dones": "u8", "ep_end": "i32"}
        self.dev = {f: m_.from_host(np.ascontiguousarray(slots[f]), kinds.get(f, "f32")) for f in FIELDS}
        K, T, N = slots["dones"].shape
        self.K, self.T, self.N, self.D = K, T, N, slots["obs"].shape[3]
        self.vec = vec

    def view(self, n_filled, **over):
        v = nat.ReplayView()
        v.n_slots, v.n_filled, v.n_steps, v.n_envs, v.obs_words = self.K, n_filled, self.T, self.N, self.D
        for name, f in (("obs", "obs"), ("actions", "actions"), ("raw_rewards", "raw"), ("dones", "dones"), ("ep_end", "ep_end"),
                        ("achieved", "ach"), ("desired", "des")):
            setattr(v, name, self.vec._mem.ptr(self.dev[f]).value)
        for name, value in over.items():
            setattr(v, name, value)
        return v


OUTPUTS = (("observation", "D", "f32"), ("next_observation", "D", "f32"), ("action", 3, "f32"), ("achieved", 4, "f32"), ("desired", 4, "f32"),
           ("reward", 0, "f32"), ("done", 0, "u8"), ("index", 4, "i32"))
GUARD = 8


def guarded_outputs(vec, B, D):
    m_ = vec._mem
    out = {}
    for name, width, kind in OUTPUTS:
        width = D if width == "D" else width
        shape = (B + GUARD, width) if width else (B + GUARD,)
        fill = {"f32": np.full(shape, -777.0, np.float32), "u8": np.full(shape, 177, np.uint8), "i32": np.full(shape, -777, np.int32)}[kind]
        out[name] = m_.from_host(fill, kind)
    return out


def raw_sample(vec, spec_struct, view, strategy, B, seed, serial, p_scaled, outs, null=None):
    """The bare call -> (status, message)."""
    m_, lib = vec._mem, vec._lib
    ptrs = [NULL if name == null else m_.ptr(outs[name]) for name, _, _ in OUTPUTS]
    st = lib.fwg_replay_sample(vec._handle, ctypes.byref(spec_struct) if spec_struct is not None else None,
                               ctypes.byref(view) if view is not None else None, strategy, B, ctypes.c_uint64(seed), ctypes.c_uint32(serial),
                               ctypes.c_uint64(p_scaled), *ptrs, m_.stream())
    return st, lib.fwg_last_error().decode()


def untouched(vec, outs, first=0):
    for name, _, kind in OUTPUTS:
        got = gc.host(vec, outs[name])[first:]
        assert (got == (177 if kind == "u8" else -777)).all(), "{}: written behind row {}".format(name, first)


def call_sample(vec, spec, dslots, n_filled, strategy, B, seed, serial, p_scaled, mode=1):
    """fwg_replay_sample over uploaded slots -> host outputs (guard rows behind every output checked)."""
    outs = guarded_outputs(vec, B, dslots.D)
    st, _ = raw_sample(vec, spec.struct(mode), dslots.view(n_filled), nat.REPLAY_STRATEGIES[strategy], B, seed, serial, p_scaled, outs)
    nat.check(vec._lib, st)
    untouched(vec, outs, B)
    return {name: gc.host(vec, outs[name])[:B] for name, _, _ in OUTPUTS}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def compare(got, want, what):
    """All outputs of one call against the restatement.  Returns the worst reward error of the relabelled samples."""
    np.testing.assert_array_equal(got["index"], want["index"], err_msg=what + ": index")
    for name in ("observation", "next_observation", "action", "achieved", "desired", "done"):
        np.testing.assert_array_equal(bits(got[name]), bits(want[name]), err_msg=what + ": " + name)
    rel = want["rel"]
    np.testing.assert_array_equal(got["reward"][~rel].view(np.int32), want["reward"][~rel].astype(np.float32).view(np.int32),
                                  err_msg=what + ": rewards of unrelabelled samples")
    worst = 0.0
    if rel.any():
        assert np.isfinite(got["reward"][rel]).all(), what
        worst = float(gc.rel_err(got["reward"][rel], want["reward"][rel]).max())
        print("{}: {} relabelled, worst relative reward error {:.3g}".format(what, int(rel.sum()), worst))
        assert worst <= gc.REWARD_TOL, (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------ 2. the index
def index_case(kw, T, N):
    vec = gc.make_env(kw, gc.goal_config("default"), 1)
    ref = gc.RefReward(vec)
    dones = gc.synthetic(ref, T, N, seed=4)[4]
    if T == T_BIG and N == N_BIG:   # the columns cycle through every pattern; spans and lane blocks are crossed
        assert T > gc.SPAN and N > 128 and not dones[:, 0].any() and dones[:, 1].all() and dones[:, 7].sum() == 3
    got = call_index(vec, dones)
    np.testing.assert_array_equal(got, ref_index(dones))
    vec.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the sample
def synthetic_slots(ref, D, K=K_BIG, T=T_BIG, N=N_BIG, seeds=(0, 1, 2)):
    """K slots of gc.synthetic rollouts; observation words hold their own flat index (exact in fp32: below 2^24), so that a wrong
    row or word shows."""
    parts = [gc.synthetic(ref, T, N, seed=s) for s in seeds[:K]]
    slots = {"ach": np.stack([p[0] for p in parts]), "des": np.stack([p[1] for p in parts]), "actions": np.stack([p[2] for p in parts]),
             "raw": np.stack([p[3] for p in parts]), "dones": np.stack([p[4] for p in parts])}
    slots["ep_end"] = np.stack([ref_index(d) for d in slots["dones"]])
    size = K * (T + 1) * N * D
    assert size < 1 << 24
    slots["obs"] = np.arange(size, dtype=np.float32).reshape(K, T + 1, N, D)
    return slots


def sample_cells(kw, kind, D):
    """One configuration and observation width: n_filled 1 / 3 x the three strategies x p 0 / 2^31 / 2^32 against the restatement."""
    vec = gc.make_env(kw, replay_config(kind), N_BIG)
    ref = gc.RefReward(vec)
    assert ref.has_delta == (kind != "default_no_delta") and ref.window == (5 if ref.has_delta else 1) and ref.potential == kind.endswith("potential")
    slots = synthetic_slots(ref, D)
    dslots = DeviceSlots(vec, slots)
    seen_back = False
    for n_filled in (1, 3):
        for strategy in STRATEGIES:
            for p in P_VALUES:
                what = "{} D {} n_filled {} {} p {}".format(kind, D, n_filled, strategy, p)
                got = call_sample(vec, ref.spec, dslots, n_filled, strategy, BATCH, SEED, SERIAL, p)
                want = ref_sample(ref, slots, n_filled, strategy, BATCH, SEED, SERIAL, p)
                compare(got, want, what)
                k, t, src, rel = want["index"][:, 0], want["index"][:, 1], want["index"][:, 3], want["rel"]
                assert (k < n_filled).all() and (p > 0 or not rel.any())
                if p == 1 << 31 and n_filled == 3:   # the case cannot pass on an empty class
                    counts = [int(rel.sum())] + [int((src == c).sum()) for c in (-1, -2, -3)]
                    per_slot = [int((k == s).sum()) for s in range(3)]
                    assert min(counts[:3]) >= 32 and min(per_slot) >= 32, (what, counts, per_slot)
                    if ref.has_delta:
                        assert counts[3] >= 32, (what, counts)
                    else:
                        assert counts[3] == 0
                    if kind == "reward_mix":
                        assert tuple(counts) == CLASS_COUNTS and tuple(per_slot) == SLOT_COUNTS, (what, counts, per_slot)
                if rel.any():
                    r = src[rel].astype(np.int64)
                    if strategy == "final":
                        assert (r == want["R"][rel]).all()
                    elif strategy == "future":
                        assert (r > t[rel]).all() and (r <= want["R"][rel]).all()
                    else:
                        assert (r > want["s0"][rel]).all() and (r <= want["R"][rel]).all()
                        seen_back = seen_back or bool((r <= t[rel]).any())
                    # the goal never crosses a done: row r is behind step r - 1, and no step from the first one considered (the
                    # episode's first in the slot, or the transition itself) up to r - 1 ends an episode
                    kk, nn = k[rel], want["index"][rel, 2]
                    first = want["s0"][rel] if strategy == "episode" else t[rel]
                    crossed = [slots["dones"][a, lo:hi, b].any() for a, b, lo, hi in zip(kk[:256], nn[:256], first[:256], r[:256])]
                    assert not any(crossed), what
    assert seen_back, "the episode strategy never took a row at or before the transition"
    vec.close()


# --------------------------------------------------------------------------------------------------------- 4. determinism, serial
def determinism_case(kw):
    vec = gc.make_env(kw, replay_config("reward_mix"), N_BIG)
    ref = gc.RefReward(vec)
    dslots = DeviceSlots(vec, synthetic_slots(ref, 14))
    one = call_sample(vec, ref.spec, dslots, 3, "future", BATCH, SEED, SERIAL, 1 << 31)
    two = call_sample(vec, ref.spec, dslots, 3, "future", BATCH, SEED, SERIAL, 1 << 31)
    for name in one:
        np.testing.assert_array_equal(bits(one[name]), bits(two[name]), err_msg=name)
    other = call_sample(vec, ref.spec, dslots, 3, "future", BATCH, SEED, SERIAL + 1, 1 << 31)
    assert (other["index"][:, :3] != one["index"][:, :3]).any(axis=1).sum() > BATCH // 2
    vec.close()


# ------------------------------------------------------------------------------------------------------------ 5. the Python layer
def python_layer(kw, n=70, n_steps=6, rollouts=4, slots=3, steps_max=10):
    """Four add_rollout calls into three slots beside a twin rollout without a replay: the twin's buffers are bit-equal; slots 1, 2 and
    the overwritten slot 0 hold bit-equal copies of the right rollouts; sample() equals the restatement on the slots' contents."""
    cfg = gc.goal_config("default")
    runs = {}
    for name in ("replay", "plain"):
        vec = gc.make_env(kw, cfg, n, config_kw={"steps_max": steps_max}, seed=2)
        vec.reset()
        actor = gc.small_head(vec)
        log = GoalLog(vec, n_steps)
        runs[name] = (vec, actor, FusedRollout(vec, actor, n_steps, raw_rewards=True, goals=log), log)
    vec, _, ro, log = runs["replay"]
    replay = HindsightReplay(vec, n_steps, slots, strategy="future", p=0.8, seed=11, target_observations="stale")
    assert replay.filled == 0 and len(replay) == 0
    kept = {}
    for r in range(rollouts):
        bufs = {name: {k: gc.host(v, b) for k, b in ro_.run().items()} for name, (v, _, ro_, _) in runs.items()}
        for k in bufs["plain"]:
            np.testing.assert_array_equal(bufs["replay"][k].view(np.uint8), bufs["plain"][k].view(np.uint8), err_msg="rollout {} buffer {}".format(r, k))
        assert replay.add_rollout(ro) == r % slots and replay.count == r + 1
        assert replay.filled == min(r + 1, slots) and len(replay) == replay.filled * n_steps * n
        kept[r % slots] = dict(bufs["replay"], last_obs=gc.host(vec, ro.cur["obs"]), ach=gc.host(vec, log.achieved), des=gc.host(vec, log.desired))
    stored = {"obs": gc.host(vec, replay.obs), "actions": gc.host(vec, replay.actions), "raw": gc.host(vec, replay.raw_rewards),
              "dones": gc.host(vec, replay.dones), "ep_end": gc.host(vec, replay.ep_end), "ach": gc.host(vec, replay.achieved),
              "des": gc.host(vec, replay.desired)}
    for k in range(slots):   # (slot 0 holds rollout 3, slots 1 and 2 rollouts 1 and 2)
        b = kept[k]
        for got, want, what in ((stored["obs"][k, :n_steps], b["obs"], "obs"), (stored["obs"][k, n_steps], b["last_obs"], "last obs"),
                                (stored["actions"][k], b["actions"], "actions"), (stored["raw"][k], b["raw_rewards"], "raw rewards"),
                                (stored["dones"][k], b["dones"], "dones"), (stored["ach"][k], b["ach"], "achieved"), (stored["des"][k], b["des"], "desired")):
            np.testing.assert_array_equal(bits(got), bits(want), err_msg="slot {}: {}".format(k, what))
        np.testing.assert_array_equal(stored["ep_end"][k], ref_index(b["dones"]), err_msg="slot {}: ep_end".format(k))
    assert stored["dones"].any() and (stored["dones"] == 0).any()
    ref = gc.RefReward(vec)
    for call in range(2):
        out = replay.sample(1000)
        assert replay.serial == call + 1
        got = {name: gc.host(vec, out[name]) for name in ("observation", "next_observation", "action", "reward", "done", "index")}
        got["achieved"], got["desired"] = gc.host(vec, out["achieved_rows"]), gc.host(vec, out["desired_rows"])
        want = ref_sample(ref, stored, slots, "future", 1000, 11, call, replay.p_scaled)
        compare(got, want, "sample {}".format(call))
        assert want["rel"].sum() >= 100 and tuple(out["desired_goal"].shape) == (1000, 3) and tuple(out["achieved_goal"].shape) == (1000, 3)
        np.testing.assert_array_equal(gc.host(vec, out["desired_goal"]), got["desired"][:, :3])
    for v, actor, _, _ in runs.values():
        actor.close()
        v.close()


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def raises(fn, word):
    try:
        fn()
    except ValueError as e:
        assert word in str(e), (word, str(e))
        return str(e)
    raise AssertionError("no ValueError holding '{}'".format(word))


def refusals(kw):
    """-> {name: message}.  The C calls return FWG_ERR_INVALID with a message that starts with their name and launch nothing (the
    outputs keep their sentinels); the Python layer raises ValueError naming the cause."""
    res = {}
    T, N, D, B = 4, 3, 8, 16
    vec = gc.make_env(kw, gc.goal_config("default"), N)
    ref = gc.RefReward(vec)
    slots = synthetic_slots(ref, D, K=2, T=T, N=N, seeds=(0, 1))
    dslots = DeviceSlots(vec, slots)
    good = ref.spec.struct(1)
    m_ = vec._mem

    def c_refusal(name, **kwargs):
        outs = guarded_outputs(vec, B, D)
        args = dict(spec_struct=good, view=dslots.view(2), strategy=0, B=B, seed=1, serial=0, p_scaled=1 << 32, outs=outs)
        args.update(kwargs)
        st, msg = raw_sample(vec, **args)
        m_.sync()
        assert st == -1 and msg.startswith("fwg_replay_sample"), (name, st, msg)
        untouched(vec, outs)
        res[name] = msg

    c_refusal("n_filled 0", view=dslots.view(0))
    c_refusal("n_filled beyond the slots", view=dslots.view(3))
    c_refusal("unknown strategy", strategy=3)
    c_refusal("negative strategy", strategy=-1)
    c_refusal("obs_words 0", view=dslots.view(2, obs_words=0))
    c_refusal("obs_words 241", view=dslots.view(2, obs_words=241))
    c_refusal("another n_envs", view=dslots.view(2, n_envs=N + 1))
    c_refusal("n_steps 0", view=dslots.view(2, n_steps=0))
    c_refusal("batch 0", B=0)
    c_refusal("batch 2^32", B=1 << 32)
    c_refusal("p_scaled", p_scaled=(1 << 32) + 1)
    c_refusal("null spec", spec_struct=None)
    c_refusal("null view", view=None)
    c_refusal("null buffer", view=dslots.view(2, ep_end=None))
    c_refusal("null output", null="reward")
    bad = ref.spec.struct(1)
    bad.n_goals = 0
    c_refusal("n_goals 0", spec_struct=bad)
    # the index call
    out = m_.from_host(np.full((T, N), -777, np.int32), "i32")
    dn = m_.from_host(np.zeros((T, N), np.uint8), "u8")
    for name, args in (("index: null", (T, N, NULL, m_.ptr(out))), ("index: n_steps 0", (0, N, m_.ptr(dn), m_.ptr(out))),
                       ("index: n_envs 0", (T, 0, m_.ptr(dn), m_.ptr(out)))):
        st = vec._lib.fwg_replay_index(*args, m_.stream())
        msg = vec._lib.fwg_last_error().decode()
        assert st == -1 and msg.startswith("fwg_replay_index"), (name, st, msg)
        res[name] = msg
    m_.sync()
    assert (gc.host(vec, out) == -777).all()
    # the Python layer: a goal state's target entry in the observation (the default preset has all three)
    res["target entry"] = raises(lambda: HindsightReplay(vec, T, 2), "type 'target'")
    assert "roll" in res["target entry"]
    replay = HindsightReplay(vec, T, 2, target_observations="stale")
    res["empty"] = raises(lambda: replay.sample(B), "empty")
    res["strategy name"] = raises(lambda: HindsightReplay(vec, T, 2, strategy="random", target_observations="stale"), "unknown strategy")
    log = GoalLog(vec, T)
    z = lambda *s: m_.zeros(s)
    fine = dict(obs=z(T, N, vec.obs_dim), last_obs=z(N, vec.obs_dim), actions=z(T, N, 3), raw_rewards=z(T, N), dones=m_.zeros((T, N), "u8"), log=log)
    for name, wrong in (("obs", z(T, N, vec.obs_dim + 1)), ("last_obs", z(N + 1, vec.obs_dim)), ("actions", z(T + 1, N, 3)), ("dones", m_.zeros((T, N + 1), "u8"))):
        res["add: " + name] = raises(lambda: replay.add(**dict(fine, **{name: wrong})), name)
    assert replay.count == 0
    raises(lambda: replay.add(**dict(fine, log=GoalLog(vec, T + 1))), "log.achieved")
    assert replay.add(**fine) == 0 and replay.filled == 1
    vec.close()
    # without the target entries the default refuses nothing
    cfg = gc.goal_config("default")
    cfg["observation"]["states"] = [s for s in cfg["observation"]["states"] if s.get("type") != "target"]
    v2 = gc.make_env(kw, cfg, N)
    assert HindsightReplay(v2, T, 2).obs_dim == v2.obs_dim == 11
    v2.close()
    # a moving target: refused where the spec is built and by the C call
    cfg, _, _, word = gc.refusal_configs()["dynamic targets"]
    v3 = gc.make_env(kw, cfg, N)
    res["moving target"] = raises(lambda: HindsightReplay(v3, T, 2, target_observations="stale"), word)
    names = [g["name"] for g in cfg["observation"]["goals"]]
    spec = GoalSpec(names, [v3.target_names.index(x) for x in names], [0.0] * len(names), [1.0] * len(names))
    outs = guarded_outputs(v3, B, D)
    d3 = DeviceSlots(v3, slots)
    st, msg = raw_sample(v3, spec.struct(1), d3.view(2), 0, B, 1, 0, 1 << 32, outs)
    v3._mem.sync()
    assert st == -1 and msg.startswith("fwg_replay_sample") and word in msg, msg
    untouched(v3, outs)
    res["moving target (C)"] = msg
    v3.close()
    return res
