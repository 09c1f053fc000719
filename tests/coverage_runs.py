"""TEST INFRASTRUCTURE: the two long-form oracle comparisons of round 6, written once for both back ends (the HIP library on a
GPU box, the host-emulation build in the CPU suite):

  * through_time_limit -- a batch through its configuration's REAL time limit (the frozen presets run 2 000-step episodes),
    every output of step()/reset() against pooled oracles (tests/oracle_pool.py);
  * steady_state_sampled -- a large batch brought to the steady state of a long run exactly as bench.py does it (stagger_ages:
    a random 1/parts of the envs reset every steps_max/parts steps), then a window of steps in which every launch mixes ending,
    failing, early-episode and drawing lanes; all outputs of ALL envs are kept on the device, a sample of env ids is chosen
    AFTERWARDS -- every lane whose last step failed on its time-limit step, failure ends, time-limit ends, their wave
    neighbours, uniform picks -- and compared with oracles created by global env id under the same reset schedule;
  * curriculum_sampled -- the same staggered run-in at an initial curriculum level, then a window driven in chunks (eager
    step_device calls, or the replay of a captured graph of them: ReplayedChunks) with set_curriculum_level between chunks;
    the checked env ids are the lanes on which a stale prepared reset draw would show (see there)."""
import copy

import numpy as np

import oracle_pool as op
import parity


def jumpy_actions(seed, steps, n, scale=1.3, p_jump=0.3):
    rng = np.random.default_rng(seed)
    a = np.zeros((steps, n, 3), dtype=np.float32)
    cur = rng.uniform(-1, 1, size=(n, 3))
    for t in range(steps):
        jump = rng.uniform(size=(n, 1)) < p_jump
        cur = np.where(jump, np.clip(cur + rng.normal(0, 0.4, size=(n, 3)), -scale, scale), cur)
        a[t] = cur
    return a


def through_time_limit(vec, cfg, ckw, skw, seed, steps, anchor_every=250, rtol=4e-3, atol=4e-3, actions=None, workers=None,
                       what=""):
    """`vec`: as_numpy=True, freshly constructed with `seed`.  Returns compare()'s summary."""
    n = vec.num_envs
    acts = jumpy_actions(5, steps, n) if actions is None else actions
    rec = op.record_run(vec, acts, anchor_every=anchor_every)
    tr = op.run_traces(copy.deepcopy(cfg), list(range(vec.env_id_base, vec.env_id_base + n)), acts, seed, config_kw=ckw,
                       sim_config_kw=skw, anchors=rec["anchors"], workers=workers)
    return op.compare(rec, tr, rtol, atol, what=what)


# ----------------------------------------------------------------------------------------------------------------------
def _is_dev(x):
    return hasattr(x, "cpu")


def _clone(x):
    return x.clone() if hasattr(x, "clone") else np.array(x)


def _at(x, pos, axis=0):
    """x[pos] along the first axis, or x[:, pos] (torch or numpy)."""
    idx = np.asarray(pos)
    if _is_dev(x):
        import torch
        idx = torch.as_tensor(idx, device=x.device)
    return x[idx] if axis == 0 else x[:, idx]


def _take(buf, w, pos):
    """buf[w][pos] as a float64 / native host array (torch or numpy buffers)."""
    x = _at(buf[w], pos)
    return x.cpu().numpy() if _is_dev(x) else np.asarray(x)


def _sim_rows(vec):
    """The eight simulator row groups [8, N, 4] of every env (a view of the state arena: y, Dryden states, gust)."""
    g0 = vec.layout.sim >> 2
    return vec.state[g0:g0 + 8]


class _Run(object):
    """What the sampled runs share: the pool of actions, the staggered run-in, the window's buffers on the device, the choice
    of env ids and the comparison of their records with the oracles."""

    def __init__(self, vec, pool_size, anchor_every):
        self.vec, self.m, self.N, self.D = vec, vec._mem, vec.num_envs, vec.obs_dim
        self.pool_size, self.anchor_every = pool_size, anchor_every
        rng = np.random.default_rng(1234)
        self.pool_h = [rng.uniform(-1, 1, (self.N, 3)).astype(np.float32) for _ in range(pool_size)]
        self.pool_d = [self.m.from_host(p) for p in self.pool_h]
        self.perm = np.random.RandomState(4321).permutation(self.N)
        self.anchors_all, self.resets_at = {}, {}
        self.g = 0            # global step: the index of the NEXT step
        self.g0 = None        # ... at which the window starts
        self.run_in_done = []  # `done` of every env at every run-in step (host copies are made at the end)

    def action(self, g):
        return self.pool_d[g % self.pool_size]

    def is_anchor(self, g):
        return bool(self.anchor_every) and g % self.anchor_every == self.anchor_every - 1

    def run_in(self, parts, per, keep_done=False):
        """bench.py's stagger_ages: a random 1/parts of the envs reset every `per` steps (parts = 0: none); then one step more if
        that leaves the window at an odd step."""
        vec, N, D = self.vec, self.N, self.D
        ro = vec.reset()
        self.reset_obs0 = ro.reshape(N, D).clone() if hasattr(ro, "clone") else np.array(ro).reshape(N, D)

        def one():
            _, _, d = vec.step_device(self.action(self.g), want_obs=False)
            if keep_done:
                self.run_in_done.append(_clone(d))
            if self.is_anchor(self.g):
                self.anchors_all[self.g] = _clone(_sim_rows(vec))
            self.g += 1

        for k in range(parts):
            idx = np.sort(self.perm[k::parts])
            self.resets_at[self.g] = idx
            vec.reset(indices=idx)
            for _ in range(per):
                one()
        if self.g % 2:
            one()
        self.g0 = self.g

    def alloc_window(self, W, rows=False):
        m, N, D = self.m, self.N, self.D
        self.obs_b, self.tobs_b = m.zeros((W, N, D)), m.zeros((W, N, D))
        self.rew_b, self.done_b, self.term_b = m.zeros((W, N)), m.zeros((W, N), "u8"), m.zeros((W, N), "u8")
        self.rows_b = m.zeros((W, 8, N, 4)) if rows else None

    def step_and_record(self, w):
        """One eager step of the window: every output of every env into slot `w` of the window's buffers."""
        vec, N, D = self.vec, self.N, self.D
        o, r, d = vec.step_device(self.action(self.g), want_obs=True)
        self.obs_b[w] = o.reshape(N, D)
        self.tobs_b[w] = vec._term_obs
        self.rew_b[w], self.done_b[w], self.term_b[w] = r, d, vec._term
        if self.rows_b is not None:
            self.rows_b[w] = _sim_rows(vec)
        elif self.is_anchor(self.g):
            self.anchors_all[self.g] = _clone(_sim_rows(vec))
        self.g += 1

    def host_events(self, W):
        from gym_fixed_wing import _native as nat
        self.m.sync()
        self.done_h = parity._np(self.done_b[:W]).astype(bool)
        self.term_h = parity._np(self.term_b[:W])
        self.fail_ends = self.done_h & (self.term_h >= nat.TERM_VAR0)
        self.steps_ends = self.done_h & (self.term_h == nat.TERM_STEPS)

    def compare(self, pos, W, cfg, ckw, skw, seed, rtol, atol, workers, what, metr=None, curriculum=None):
        """The oracles of the env ids at `pos` -- the same life by global env id -- against the window's record of them."""
        from gym_fixed_wing import _native as nat
        vec, base, g0 = self.vec, self.vec.env_id_base, self.g0
        T = g0 + W
        acts = np.stack([self.pool_h[t % self.pool_size][pos] for t in range(T)])
        where = {int(p): j for j, p in enumerate(pos)}
        resets = {}
        for gs, idx in self.resets_at.items():
            loc = [where[int(e)] for e in idx if int(e) in where]
            if loc:
                resets[gs] = loc
        if self.rows_b is not None:   # (the window kept the rows of every step: the anchor steps among them)
            for w in range(W):
                if self.is_anchor(g0 + w):
                    self.anchors_all[g0 + w] = self.rows_b[w]
        anchors = {}
        for gs, rows in self.anchors_all.items():
            if gs >= T:
                continue
            w_ = parity._np(_at(rows, pos, axis=1))   # rows [8, N, 4] -> [8, len(pos), 4]
            w_ = w_.astype(np.float64).transpose(1, 0, 2).reshape(len(pos), 32)
            anchors[gs] = (w_[:, :18].copy(), w_[:, 18:26].copy(), w_[:, 26:32].copy())
        tr = op.run_traces(copy.deepcopy(cfg), [base + int(p) for p in pos], acts, seed, config_kw=ckw, sim_config_kw=skw,
                           resets=resets, anchors=anchors, workers=workers, keep_from=g0, curriculum=curriculum)
        done_h, term_h = self.done_h, self.term_h
        rec = {"reset_obs": parity._np(_at(self.reset_obs0, pos)).astype(np.float64),
               "obs": np.stack([_take(self.obs_b, w, pos) for w in range(W)]).astype(np.float64),
               "reward": np.stack([_take(self.rew_b, w, pos) for w in range(W)]).astype(np.float64), "done": done_h[:, pos],
               "target": np.zeros((W, len(pos), 3)), "term": {}, "term_obs": {}, "metrics": {}, "masked_reset_obs": tr["masked_reset_obs"]}
        for w, j in zip(*np.nonzero(done_h[:, pos])):
            w, j = int(w), int(j)
            rec["term"][(w, j)] = nat.term_name(term_h[w, pos[j]])
            rec["term_obs"][(w, j)] = _take(self.tobs_b, w, [pos[j]])[0].astype(np.float64)
            # metrics: collected every `metrics_every` steps; the column of an env holds its LAST finished episode
            later = [x for x in sorted(metr or {}) if x >= w]
            if later and not done_h[w + 1:later[0] + 1, pos[j]].any():
                col = parity._np(metr[later[0]])[:, pos[j]]
                rec["metrics"][(w, j)] = vec.metrics_dict(col)
        return op.compare(rec, tr, rtol, atol, what=what, check_target=False), where


class _Chosen(object):
    """The env ids to check, taken class by class: no env twice (an env checked twice would get its masked reset once)."""

    def __init__(self, N, sample, select_seed):
        self.N, self.sample, self.rng, self.ids = N, sample, np.random.default_rng(select_seed), []

    def add(self, cands, k):
        chosen = self.ids
        k = min(k, self.sample - len(chosen))
        if k <= 0:
            return
        cands = list(dict.fromkeys(int(c) for c in cands if int(c) not in set(chosen)))
        if len(cands) > k:
            cands = list(self.rng.choice(cands, size=k, replace=False))
        chosen.extend(int(c) for c in cands)

    def add_neighbours(self, k):
        chosen, N = self.ids, self.N
        neigh = [e ^ 1 for e in chosen if (e ^ 1) < N] + [min(N - 1, (e & ~63) + int(self.rng.integers(64))) for e in chosen]
        self.add(neigh, k)

    def fill_uniform(self):
        self.add(self.rng.choice(self.N, size=min(self.N, 4 * self.sample), replace=False), self.sample - len(self.ids))

    def positions(self):
        pos = np.array(sorted(self.ids[:self.sample]))
        assert len(set(pos.tolist())) == len(pos)
        return pos


def steady_state_sampled(vec, cfg, ckw, skw, seed, window=300, parts=None, sample=256, pool_size=8, anchor_every=10,
                         rtol=4e-3, atol=4e-3, workers=None, what="", metrics_every=100, select_seed=0, first_pick=None):
    """`vec`: device tensors (as_numpy=False) or the emulation backend, auto_reset=True, freshly constructed with `seed`.
    parts = 0: no run-in -- the window starts at the reset of a fresh VecEnv, all episodes in LOCK-STEP (the regime of a real
    run's time-limit ends: whole cohorts of lanes end in one launch, next to lanes that failed earlier and are at other ages).
    Anchors every 10 steps (oracle_pool.trace_envs): full-scale independent random commands on 65 536 aircraft find the
    tumbling / diving ones (Va 43 m/s on its way to the airspeed constraint), whose float32 and float64 trajectories separate by
    1e-2 within fifty steps -- and the lagged rows of an observation carry the drift of before an anchor for eight more steps."""
    N = vec.num_envs
    steps_max = int(vec.cfg["steps_max"])
    parts = steps_max if parts is None else int(parts)
    per = max(1, steps_max // max(parts, 1))
    run = _Run(vec, pool_size, anchor_every)
    run.run_in(parts, per)   # ---- the run-in: bench.py's stagger_ages
    g0 = run.g0
    # ---- the window: everything every env returns, kept on the device (65 536 envs x 300 steps x 60 floats = 4.7 GB, twice)
    W = int(window)
    run.alloc_window(W)
    metr = {}
    for w in range(W):
        run.step_and_record(w)
        if metrics_every and (w % metrics_every == metrics_every - 1 or w == W - 1):
            metr[w] = _clone(vec.metrics())
    run.host_events(W)
    done_h, fail_ends, steps_ends = run.done_h, run.fail_ends, run.steps_ends
    # ---- which envs to check: chosen from what happened
    first_reset = np.zeros(N, dtype=np.int64)
    for gs, idx in run.resets_at.items():
        first_reset[idx] = gs
    limit_w = first_reset + steps_max - 1 - g0          # window step on which an env reset at first_reset runs out of time
    ws = np.arange(W)[:, None]
    fail_on_limit = np.nonzero((fail_ends & (ws == limit_w[None, :])).any(axis=0))[0]
    ch = _Chosen(N, sample, select_seed)
    picked_first = 0
    if first_pick is not None:   # (a test's own class of lanes: first_pick(fail_ends [W, N], steps_ends [W, N], g0) -> env ids)
        ch.add(first_pick(fail_ends, steps_ends, g0), sample // 4)
        picked_first = len(ch.ids)
    ch.add(fail_on_limit, sample // 4)
    ch.add(np.nonzero(fail_ends.any(axis=0))[0], sample // 4)
    ch.add(np.nonzero(steps_ends.any(axis=0))[0], sample // 4)
    ch.add_neighbours(sample // 8)
    ch.fill_uniform()
    pos = ch.positions()
    # ---- the oracles: the same life by global env id; the product's record of the same envs over the window
    res, where = run.compare(pos, W, cfg, ckw, skw, seed, rtol, atol, workers, what, metr=metr)
    ends_per_env = done_h[:, pos].sum(axis=0)
    res.update({"sampled": len(pos), "ends_in_window": int(done_h.sum()), "failure_ends": int(fail_ends.sum()),
                "time_limit_ends": int(steps_ends.sum()), "failed_on_the_limit_step": int(len(fail_on_limit)),
                "failed_on_the_limit_step_checked": int(sum(1 for e in fail_on_limit if int(e) in where)),
                "sampled_ends": int(ends_per_env.sum()), "first_pick_checked": picked_first})
    return res


# ----------------------------------------------------------------------------------------------------------------------
# curriculum level changes in the middle of a run
# ----------------------------------------------------------------------------------------------------------------------
CLASSES = ("a", "b", "c", "d")
DRAW_READY = 6   # csrc/fwgym_env.h FWG_DRAW_READY: the stage (flags bits 4..6) of a complete prepared reset draw


def draw_stages(vec):
    """The stage of every env's prepared reset draw (0 nothing .. 6 complete), as a device / host array to be decoded later
    (draw_stages_np): flags word of the bookkeeping block, bits 4..6."""
    return _clone(vec.state[(vec.layout.gym >> 2) + 1][:, 0])


def draw_stages_np(words):
    return (np.ascontiguousarray(parity._np(words)).view(np.uint32) >> 4) & 7


class EagerChunks(object):
    """The window's stepper in its plain form: `k` direct step_device calls.  Chunks of any length."""
    fixed_chunk = False

    def __call__(self, run, w, k):
        for i in range(k):
            run.step_and_record(w + i)
        return k


class ReplayedChunks(object):
    """The window's stepper as a graphed learner drives the env (rollout.GraphedRollout): `chunk` step_device calls captured
    ONCE into a hipGraph (torch.cuda.CUDAGraph; one stream: no parallel branches) -- actions read from fixed device buffers
    that are refilled before every replay, every output copied into per-chunk buffers inside the capture -- and replayed under
    replay_check / note_replayed_steps.  Where replay_check refuses, the recipe of its message: two direct steps (they count:
    the chunk is then chunk + 2 steps long), then a new capture.  `refusals`: [(window step, message)]."""
    fixed_chunk = True

    def __init__(self, vec, chunk):
        import torch
        assert chunk % 2 == 0
        self.torch, self.vec, self.chunk = torch, vec, int(chunk)
        self.graph, self.token = None, None
        self.refusals, self.captures, self.instances = [], 0, []

    def _begin(self):
        """Graph mode from the window's first chunk on, as a learner enters it: after the resets of the run-in."""
        vec, chunk = self.vec, self.chunk
        m, N, D = vec._mem, vec.num_envs, vec.obs_dim
        vec.set_graph_mode(True)
        self.acts = [m.zeros((N, 3)) for _ in range(chunk)]
        self.out = {"obs": m.zeros((chunk, N, D)), "tobs": m.zeros((chunk, N, D)), "rew": m.zeros((chunk, N)),
                    "done": m.zeros((chunk, N), "u8"), "term": m.zeros((chunk, N), "u8"), "rows": m.zeros((chunk, 8, N, 4))}

    def _record(self, i):
        vec, out = self.vec, self.out
        o, r, d = vec.step_device(self.acts[i], want_obs=True)
        out["obs"][i].copy_(o.reshape(vec.num_envs, vec.obs_dim))
        out["tobs"][i].copy_(vec._term_obs)
        out["rew"][i].copy_(r)
        out["done"][i].copy_(d)
        out["term"][i].copy_(vec._term)
        out["rows"][i].copy_(_sim_rows(vec))

    def _capture(self):
        torch, vec = self.torch, self.vec
        dev = vec._mem.device
        for k, v in self.out.items():   # (every copy kernel of the body has run once before the capture; no env step)
            v[0].copy_(v[1])
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        self.token = vec.capture_begin(self.chunk)
        with torch.cuda.graph(graph):
            for i in range(self.chunk):
                self._record(i)
        vec.capture_end()
        self.graph = graph
        self.captures += 1
        self.instances.append(vec.spec_index)

    def __call__(self, run, w, k):
        from gym_fixed_wing import _native as nat
        assert k == self.chunk, (k, self.chunk)
        vec, n = self.vec, 0
        if self.graph is None:
            self._begin()
            self._capture()
        else:
            try:
                vec.replay_check(self.token)
            except nat.NativeError as err:
                self.refusals.append((w, str(err)))
                run.step_and_record(w)
                run.step_and_record(w + 1)
                n = 2
                self._capture()
                vec.replay_check(self.token)
        for i in range(k):
            self.acts[i].copy_(run.action(run.g + i))
        self.graph.replay()
        vec.note_replayed_steps(k)
        lo = w + n
        run.obs_b[lo:lo + k].copy_(self.out["obs"])
        run.tobs_b[lo:lo + k].copy_(self.out["tobs"])
        run.rew_b[lo:lo + k].copy_(self.out["rew"])
        run.done_b[lo:lo + k].copy_(self.out["done"])
        run.term_b[lo:lo + k].copy_(self.out["term"])
        run.rows_b[lo:lo + k].copy_(self.out["rows"])
        run.g += k
        return n + k


def curriculum_classes(done_h, fail_ends, steps_ends, start_g, g0, changes, W, stages=None):
    """The lanes on which a wrongly kept reset draw would show, per level change (`changes`: the window steps before which a
    level was set; `start_g` [N]: the global step of the first step of the episode each env was in when the window began):
      a  the time limit falls on the FIRST step after the change: the episode end was foreseen, the prepared draw is complete
         and of the old generation -- the two waves' decision whether the physics wave installs the next episode (pre_install);
      b  the episode was 1-4 steps old at the change: its successor's draw is half prepared under the old generation;
      c  the first end after the change is a FAILURE end: not foreseen, the gym wave's own check of the tag;
      d  two ends or more between this change and the next: the second draw is prepared wholly under the new generation.
    A prepared draw advances by one piece per step only in waves that host no episode end in that step, the least advanced lanes
    first: where every wave hosts an end in most steps (45-step episodes, 64 lanes) no draw is ever completed and every reset
    draws on the spot, with the ranges of the moment -- a run there cannot show a stale draw.  So, with `stages` {change: stage
    [N] of every env's draw at the change}, the classes are also counted by what the lanes actually held:
      a_ready  a, with a COMPLETE draw at the change;
      c_ready  c, with a complete draw at the change;
      half     a draw of 1-5 pieces at the change (whatever the age), and an end before the next change.
    Returns {change: {class: env ids}}."""
    N = done_h.shape[1]
    out = {}
    ch = sorted(changes)
    for i, s in enumerate(ch):
        nxt = ch[i + 1] if i + 1 < len(ch) else W
        # age at the change: steps the running episode has made
        start = np.asarray(start_g, dtype=np.int64) - g0           # (window step of the episode's first step; negative: before it)
        if s > 0:
            any_before = done_h[:s].any(axis=0)
            last = s - 1 - np.argmax(done_h[:s][::-1], axis=0)    # last end before the change
            start = np.where(any_before, last + 1, start)
        age = s - start
        after = done_h[s:nxt]
        has_end = after.any(axis=0)
        first = s + np.argmax(after, axis=0)
        out[s] = {"a": np.nonzero(steps_ends[s])[0] if s < W else np.zeros(0, dtype=np.int64),
                  "b": np.nonzero((age >= 1) & (age <= 4))[0],
                  "c": np.nonzero(has_end & fail_ends[np.minimum(first, W - 1), np.arange(N)])[0],
                  "d": np.nonzero(after.sum(axis=0) >= 2)[0]}
        if stages is not None:
            st = stages[s]
            ready = np.nonzero(st == DRAW_READY)[0]
            out[s]["a_ready"] = np.intersect1d(out[s]["a"], ready)
            out[s]["c_ready"] = np.intersect1d(out[s]["c"], ready)
            out[s]["half"] = np.nonzero((st >= 1) & (st < DRAW_READY) & has_end)[0]
            out[s]["ready_lanes"] = ready
    return out


def _class_picks(sample, n_changes):
    """How the sample is shared out, per level change: class a 5/32 of it, c 5/32, b 2/32, lanes with a half-prepared draw 1/32,
    d 2/32 (two changes; twice that with one, less with more).  Within a class the lanes that HELD a complete / a half-prepared
    draw at the change come first.  Returns functions: classes of one change -> (candidate env ids, how many to take)."""
    share = 2.0 / max(1, n_changes)

    def quota(parts_of_32):
        return max(1, int(sample * parts_of_32 // 32 * share))

    def a_ready(c):
        return c["a_ready"], quota(5)

    def a_rest(c):
        return c["a"], quota(5) - len(c["a_ready"])

    def c_ready(c):
        return c["c_ready"], quota(5) // 2

    def c_rest(c):
        return c["c"], quota(5) - min(quota(5) // 2, len(c["c_ready"]))

    def b_half(c):
        return np.intersect1d(c["b"], c["half"]), quota(2)

    def b_rest(c):
        return c["b"], max(quota(2) // 4, quota(2) - len(np.intersect1d(c["b"], c["half"])))

    def half(c):
        return c["half"], quota(1)

    def d(c):
        return c["d"], quota(2)

    return [a_ready, a_rest, c_ready, c_rest, b_half, b_rest, half, d]


def curriculum_sampled(vec, cfg, ckw, skw, seed, level0, schedule, window=96, chunk=16, stepper=None, sample=64, parts=None,
                       run_in_steps=0, pool_size=8, anchor_every=10, rtol=4e-3, atol=4e-3, workers=None, what="", select_seed=0,
                       keep_buffers=False, compare=True):
    """set_curriculum_level in the middle of a run (what PPO.learn's CurriculumSchedule does between rollouts).  `vec` as for
    steady_state_sampled.  Level `level0` is set before the first reset; the run-in staggers the ages exactly as
    steady_state_sampled does (parts = 0: lock-step, then `run_in_steps` plain steps), so that every launch of the window hosts
    lanes of every age; the window is driven in chunks of `chunk` steps (an int, or the list of chunk lengths) by `stepper`
    (EagerChunks, ReplayedChunks); `schedule` {window step: level} is applied between chunks -- an EagerChunks window ends a chunk
    early so that a change lands on its step, a stepper of fixed chunks gets the change at the first chunk boundary at or after
    it (`applied` in the summary: where the changes went; `chunks`: the lengths driven).  The same schedule, shifted by the
    run-in, goes to the oracles.  All outputs of all envs stay on the device; the env ids are chosen AFTERWARDS, per change
    the classes of curriculum_classes first, then their wave neighbours, then uniform picks.  The summary carries, beside
    what steady_state_sampled returns, `classes` {change: {class: checked, class_all: lanes of the class in the batch}};
    with keep_buffers, `buffers`: the window's record of ALL envs (device arrays)."""
    N = vec.num_envs
    steps_max = int(vec.cfg["steps_max"])
    parts = steps_max if parts is None else int(parts)
    per = max(1, steps_max // max(parts, 1))
    stepper = EagerChunks() if stepper is None else stepper
    vec.set_curriculum_level(level0)
    run = _Run(vec, pool_size, anchor_every)
    run.run_in(parts, per, keep_done=True)
    for _ in range(int(run_in_steps) & ~1):
        _, _, d = vec.step_device(run.action(run.g), want_obs=False)
        run.run_in_done.append(_clone(d))
        if run.is_anchor(run.g):
            run.anchors_all[run.g] = _clone(_sim_rows(vec))
        run.g += 1
    run.g0 = g0 = run.g
    # ---- the window, in chunks, the level changes between them
    W = int(window)
    lengths = list(chunk) if isinstance(chunk, (list, tuple)) else None
    cmax = max(lengths) if lengths else int(chunk)
    run.alloc_window(W + cmax + 2 * (len(schedule) + 1), rows=True)
    pending = sorted((int(s), float(l)) for s, l in schedule.items())
    applied, chunks, stages, w = {}, [], {}, 0
    while w < W:
        while pending and pending[0][0] <= w:
            stages[w] = draw_stages(vec)
            vec.set_curriculum_level(pending[0][1])
            applied[w] = pending.pop(0)[1]
        k = lengths[len(chunks)] if lengths else int(chunk)
        if not stepper.fixed_chunk and pending:
            k = min(k, pending[0][0] - w)
        n = stepper(run, w, k)
        chunks.append(n)
        w += n
    W = w
    run.host_events(W)
    done_h, fail_ends, steps_ends = run.done_h, run.fail_ends, run.steps_ends
    # ---- the episode every env was in when the window began: the masked resets and the ends of the run-in
    start_g = np.zeros(N, dtype=np.int64)
    for gs, idx in sorted(run.resets_at.items()):
        start_g[idx] = gs
    if run.run_in_done:
        rd = np.stack([parity._np(d) for d in run.run_in_done]).astype(bool)   # [g0, N]
        last_end = rd.shape[0] - 1 - np.argmax(rd[::-1], axis=0)
        start_g = np.where(rd.any(axis=0), np.maximum(start_g, last_end + 1), start_g)
    stages = {s: draw_stages_np(v) for s, v in stages.items()}
    cls = curriculum_classes(done_h, fail_ends, steps_ends, start_g, g0, list(applied), W, stages)
    # ---- which envs to check
    ch = _Chosen(N, sample, select_seed)
    for group in _class_picks(sample, len(applied)):   # class by class over all changes: a small sample is not used up by the first
        for s in sorted(cls):
            ids, k = group(cls[s])
            ch.add(ids, max(1, k))
    ch.add_neighbours(sample // 8)
    ch.fill_uniform()
    pos = ch.positions()
    curriculum = {-1: level0}
    curriculum.update({g0 + s: lvl for s, lvl in applied.items()})
    if compare:
        res, where = run.compare(pos, W, cfg, ckw, skw, seed, rtol, atol, workers, what, curriculum=curriculum)
    else:   # (the second run of a bit-by-bit comparison of two runs: its record only)
        res, where = {}, {int(p): j for j, p in enumerate(pos)}
    counts = {}
    for s in sorted(cls):
        counts[s] = {}
        for c in CLASSES + ("a_ready", "c_ready", "half"):
            counts[s][c] = int(sum(1 for e in cls[s][c] if int(e) in where))
            counts[s][c + "_all"] = int(len(cls[s][c]))
        counts[s]["ready_lanes_all"] = int(len(cls[s]["ready_lanes"]))
    res.update({"sampled": len(pos), "ends_in_window": int(done_h.sum()), "failure_ends": int(fail_ends.sum()),
                "time_limit_ends": int(steps_ends.sum()), "sampled_ends": int(done_h[:, pos].sum()), "window": W, "g0": g0,
                "applied": applied, "chunks": chunks, "classes": counts})
    if keep_buffers:   # (a caller that compares two runs bit by bit: the window's record of ALL envs)
        res["buffers"] = {"obs": run.obs_b[:W], "term_obs": run.tobs_b[:W], "reward": run.rew_b[:W], "done": run.done_b[:W],
                          "term": run.term_b[:W]}
    return res
