// fwgym_goal.h -- the goal-conditioned view of a handle and hindsight relabelling on the device (fwg_goal_observe, fwg_goal_reward,
// fwg_goal_relabel; include/fwgym.h "Goal env").
//
// The reference's FixedWingAircraftGoal (fixed_wing.py:1165-1277) is a gym.GoalEnv: dict observations with the goal states scaled
// by (x - mean) / var, and compute_reward(achieved_goal, desired_goal, info) -- get_reward re-evaluated for SUBSTITUTED goal states
// and targets, the call a hindsight replay buffer makes for every transition it relabels.  Three stateless launches over
// caller-owned buffers do that for a batch: nothing travels by value that changes from step to step (the goal description and the
// structure words of the handle only), so fwg_goal_observe sits inside a captured rollout like the flight recorder's launch.
//
// Goal rows are float4: words 0..2 the scaled goals in the spec's order (unused words 0), word 3 per buffer (include/fwgym.h).
//
// The reward function (goal_reward) restates get_reward with success = False, as gym_fixed_wing/fixed_wing.py _host_reward /
// compute_reward do in float64 (the yardstick, itself pinned to the verbatim reference by tests/golden/g4_goal_*.json):
//   * state value / error factors and the goal flags come from the UNSCALED achieved goals (values) and desired goals (targets);
//     angle-wrapped errors go through target_error as in the step; goal-class factors through goal_flags and the configured bounds;
//   * action value / delta / bound factors come from the window of raw actions, as the step computes fval_action;
//   * success-class factors contribute 0, the step class its constant;
//   * potential form: the previous shaping values are those of the goals BEFORE the transition (`prev`) against the same targets,
//     with the action before for the bound factor and -- the reference's quirk, kept -- the SAME action list for value and delta.
// It reads the handle's lowered configuration in device memory (the generic object: factor table, terms, bounds, action bounds),
// so a curriculum level or fwg_update_config is seen by the next launch.  The host refuses what the yardstick cannot define from the
// transition alone (goal_lower in fwgym.hip).
//
// k_goal_relabel is HER's "future" strategy over one step-major rollout; its semantics are normative in include/fwgym.h and restated
// in numpy by tests/goal_common.py.  Shape (k_gae's / k_monitor_fold's): a workgroup of four waves takes 64 adjacent envs x a span
// of 128 steps, wave w the segment [w L, (w + 1) L), L = 32.  A lane packs its segment's 32 done flags into one mask; the index of
// each segment's first done meets in LDS after ONE barrier, so every lane knows R (the first done after t, or T) for each of its
// transitions: inside its mask by a bit scan, else the first done of a later segment, else the carry from the later spans (spans
// are walked from the last to the first).  The four waves then decide their own 32 transitions each: the Philox draw, src, and the
// gather of the new goal into desired_out.  Lanes with e >= N load env N - 1's values (no out-of-bounds address) and store nothing.
// The reward of the relabelled transitions is a second launch, one lane per transition (k_goal_relabel_reward): it reads src and
// the new goal back (20 B) instead of carrying the reward function's registers through the scan -- in one kernel the configuration
// words, 26 words of arguments and the scan's state did not fit the scalar registers.  No atomics, no scratch, no spills.
#ifndef FWGYM_GOAL_H
#define FWGYM_GOAL_H

#define FWG_STREAM_GOAL 10u               /* Philox stream of the relabelling draws (1..9 are taken, fwgym_dev.h / fwgym_actor.h) */
#define FWG_GOAL_L 32                     /* steps per wave segment */
#define FWG_GOAL_SPAN (4 * FWG_GOAL_L)    /* steps per workgroup span */
#define FWG_GOAL_SRC_KEPT (-1)            /* the draw kept the transition's own goal */
#define FWG_GOAL_SRC_DONE (-2)            /* terminal transition: the achieved goal after it is not in the buffer */
#define FWG_GOAL_SRC_WINDOW (-3)          /* the action window reaches before row 0 of the rollout */

// the caller's fwg_goal_spec and the structure words of the handle it needs, by value (none of it changes from launch to launch)
struct GoalCfg {
    int n, mode, window, has_delta;       // goals; step_count_mode; fwg_goal_window; a delta factor exists
    int k[3], di[3];                      // per goal: target slot; index for rec_derived (0 roll, 1 pitch, 3 Va)
    float mean[3], var[3];
};
// raw actions BY AGE: a[0] the transition's own, a[j] the one j steps before it (zeros where the episode is younger)
struct GoalWin { float a[FWG_MAX_WINDOW][3]; };

__device__ __forceinline__ void goal_unscale(const GoalCfg& g, const float4& row, float (&x)[3]) {
    x[0] = row.x * g.var[0] + g.mean[0];
    x[1] = row.y * g.var[1] + g.mean[1];
    x[2] = row.z * g.var[2] + g.mean[2];
}
// errors by TARGET SLOT of goal values against goal targets (slots that are no goal: 0 -- the host refused every use of them)
__device__ __forceinline__ void goal_errors(const DevCfg& c, const GoalCfg& g, const float (&val)[3], const float (&tgt)[3], float (&err)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        err[k] = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < g.n && g.k[i] == k && k < c.n_targets) err[k] = target_error(c.target[k], tgt[i], val[i]);
    }
}
// the factor loop of get_reward (fixed_wing.py:683-751) -> per function class the plain sums nv and the shaping sums sh.
// bound_age: which action the bound factor sees (0 the transition's own, 1 the one before); step: the transition's index in its episode
__device__ __forceinline__ void goal_terms(const DevCfg& c, const GoalCfg& g, const float (&x)[3], const float (&err)[3], const GoalWin& w,
                                           int bound_age, unsigned step, float (&nv)[3], float (&sh)[3]) {
    const unsigned gf = goal_flags(c, err);
    const unsigned counter = step + (g.mode ? 1u : 0u);   // mode 0: compute_reward's steps_count = info["step"]; mode 1: step()'s
    nv[0] = nv[1] = nv[2] = 0.f;
    sh[0] = sh[1] = sh[2] = 0.f;
    for (int f = 0; f < c.n_factors; ++f) {
        const DevFactor& F = c.factor[f];
        float val = 0.f;
        if (F.cls == FWG_RC_ACTION) {
            if (F.type == FWG_RT_VALUE) val = fabsf(w.a[0][0]) + fabsf(w.a[0][1]) + fabsf(w.a[0][2]);
            else if (F.type == FWG_RT_DELTA) {
                if (counter > 1u) {
                    const int m = (int)min(step + 1u, (unsigned)F.window);   // actions of this episode the window holds
#pragma unroll
                    for (int k = FWG_MAX_WINDOW - 2; k >= 0; --k) {
                        if (k <= m - 2) {
#pragma unroll
                            for (int i = 0; i < 3; ++i) val += fabsf(w.a[k][i] - w.a[k + 1][i]);
                        }
                    }
                }
            } else if (bound_age == 0 || step >= 1u) {   // bound (no action before the first one: 0)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float a = bound_age == 0 ? w.a[0][i] : w.a[1][i];
                    val += a > c.act_bound_max[i] ? a - c.act_bound_max[i] : 0.f;
                    val += a < c.act_bound_min[i] ? c.act_bound_min[i] - a : 0.f;
                }
            }
        } else if (F.cls == FWG_RC_STATE) {
            if (F.type == FWG_RT_VALUE) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < g.n && c.target[g.k[i]].var == F.src) val = x[i];
            } else {
                val = F.src == 0 ? err[0] : (F.src == 1 ? err[1] : err[2]);
            }
        } else if (F.cls == FWG_RC_STEP) {
            val = F.value;
        } else if (F.cls == FWG_RC_GOAL) {
            if (F.type == FWG_RT_PER_STATE) {
#pragma unroll
                for (int k = 0; k < FWG_MAX_TARGETS; ++k)
                    if (k < c.n_targets && c.target[k].has_bound && ((gf >> k) & 1u)) val += F.value / (float)c.n_targets;
            } else {
                val = (gf & 8u) ? F.value : 0.f;
            }
        }   // (success class: 0 -- success = False)
        if (F.fclass == FWG_FC_LINEAR) {
            val = fabsf(val) * F.inv_scaling;
            if (F.has_max) val = fminf(val, F.max);
        } else {
            val = val * val * F.inv_scaling;
        }
        val *= F.sign;
        const int fc = F.fclass;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            sh[i] += (i == fc && F.shaping) ? val : 0.f;
            nv[i] += (i == fc && !F.shaping) ? val : 0.f;
        }
    }
}
// compute_reward (fixed_wing.py:1218-1277) for one transition.  ach / des / prv: scaled goal rows (prv is read only in the
// potential form and only when step > 0)
__device__ __forceinline__ float goal_reward(const DevCfg& c, const GoalCfg& g, const float4& ach, const float4& des, const float4& prv,
                                             const GoalWin& w, unsigned step) {
    float x[3], tg[3], err[3], nv[3], sh[3], psh[3] = {0.f, 0.f, 0.f};
    goal_unscale(g, des, tg);
    const bool has_prev = c.reward_potential && step > 0u;
    if (has_prev) {
        float pn[3];
        goal_unscale(g, prv, x);
        goal_errors(c, g, x, tg, err);
        goal_terms(c, g, x, err, w, 1, step, pn, psh);
    }
    goal_unscale(g, ach, x);
    goal_errors(c, g, x, tg, err);
    goal_terms(c, g, x, err, w, 0, step, nv, sh);
    float reward = 0.f;
#pragma unroll
    for (int fc = 0; fc < 3; ++fc) {
        if (c.term_present[fc]) {
            float v = nv[fc];
            if (c.reward_potential) { if (has_prev) v += sh[fc] - psh[fc]; }
            else v += sh[fc];
            if (fc == FWG_FC_EXPONENTIAL) v = expf(v) - 1.f;
            reward += c.term_weight[fc] * v;
        }
    }
    return reward;
}

// the goal rows of env e: the committed state and the current targets (k_goal_observe, and the behaviour head of fwgym_behaviour.h)
__device__ __forceinline__ void goal_rows_of(const RecCfg& rc, const GoalCfg& g, const float* __restrict__ S, long N, long e, float4& achieved,
                                             float4& desired) {
    float a[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < g.n) {
            a[i] = (rec_derived(rc, S, N, e, g.di[i]) - g.mean[i]) / g.var[i];
            d[i] = (rec_arena(S, N, e, rc.gym + g.k[i]) - g.mean[i]) / g.var[i];
        }
    }
    achieved = make_float4(a[0], a[1], a[2], rec_arena(S, N, e, rc.gym + 3));   // word 3: the step word, as bits
    desired = make_float4(d[0], d[1], d[2], 0.f);
}

// one lane per env
__global__ __launch_bounds__(256) void k_goal_observe(RecCfg rc, GoalCfg g, const float* __restrict__ S, long N, float4* __restrict__ achieved,
                                                      float4* __restrict__ desired) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    float4 a, d;
    goal_rows_of(rc, g, S, N, e, a, d);
    achieved[e] = a;
    desired[e] = d;
}

// one lane per transition: act_win [W][m] rows (a0 a1 a2 -), row W - 1 the transition's own action
__global__ __launch_bounds__(256) void k_goal_reward(const DevCfg* __restrict__ cfg, GoalCfg g, long m, const float4* __restrict__ achieved,
                                                     const float4* __restrict__ desired, const float4* __restrict__ prev,
                                                     const float4* __restrict__ act_win, const int* __restrict__ step, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const DevCfg& c = *cfg;
    const int st = step[i];
    const unsigned s = st < 0 ? 0u : (unsigned)st;
    GoalWin w;
#pragma unroll
    for (int j = 0; j < FWG_MAX_WINDOW; ++j) {
        w.a[j][0] = w.a[j][1] = w.a[j][2] = 0.f;
        if (j < g.window && (unsigned)j <= s) {   // (rows older than `step` actions back are never read)
            const float4 q = act_win[(long)(g.window - 1 - j) * m + i];
            w.a[j][0] = q.x; w.a[j][1] = q.y; w.a[j][2] = q.z;
        }
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 pv = (c.reward_potential && s > 0u) ? prev[i] : zero;
    out[i] = goal_reward(c, g, achieved[i], desired[i], pv, w, s);
}

struct GoalRelabel {
    const float4* achieved;   // [T + 1][N]
    const float4* desired;    // [T + 1][N]
    const float* actions;     // [T][N][3]
    const float* raw;         // [T][N]
    const unsigned char* done;   // [T][N]
    float4* desired_out;      // [T][N]
    float* reward_out;        // [T][N]
    int* src_out;             // [T][N]
    long T, N;
    unsigned env_base, serial, seed_lo, seed_hi;
    unsigned long long p_scaled;
};

// launch 1 of fwg_goal_relabel: the integer decisions and the goal gather (no reward arithmetic, no configuration read)
__global__ __launch_bounds__(256) void k_goal_relabel(GoalCfg g, GoalRelabel A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int* const first = reinterpret_cast<int*>(lds);   // [4 waves][64 lanes]: step of the segment's first done, or -1
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long T = A.T, N = A.N;
    const long e0 = (long)blockIdx.x * 64 + lane;
    const bool valid = e0 < N;
    const long e = valid ? e0 : N - 1;
    long carry = T;   // the first done of the spans after this one (every lane keeps its own copy), or T
    for (long lo = ((T - 1) / FWG_GOAL_SPAN) * FWG_GOAL_SPAN; lo >= 0; lo -= FWG_GOAL_SPAN) {
        const long hi = lo + FWG_GOAL_SPAN < T ? lo + FWG_GOAL_SPAN : T;
        const long s0 = lo + (long)w * FWG_GOAL_L;   // this wave's segment [s0, s1) (empty past the end of a short span)
        const long s1 = s0 + FWG_GOAL_L < hi ? s0 + FWG_GOAL_L : hi;
        unsigned mask = 0u;
#pragma unroll
        for (int k = 0; k < FWG_GOAL_L; ++k)
            if (s0 + k < s1) mask |= A.done[(s0 + k) * N + e] != 0 ? (1u << k) : 0u;
        first[w * 64 + lane] = mask != 0u ? (int)(s0 + (__ffsll((long long)mask) - 1)) : -1;
        __syncthreads();
        long after = carry;   // the first done after this wave's segment
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const int fj = first[j * 64 + lane];
            if (fj >= 0) {
                carry = fj;
                if (j > w) after = fj;
            }
        }
        __syncthreads();   // the summaries are read before the next span overwrites them
        for (int k = 0; k < FWG_GOAL_L; ++k) {
            const long t = s0 + k;
            if (t >= s1 || !valid) continue;
            const unsigned later = k < FWG_GOAL_L - 1 ? mask >> (k + 1) : 0u;
            const long R = later != 0u ? t + __ffsll((long long)later) : after;   // first t_e > t with a done, or T
            const unsigned idx = __float_as_uint(A.achieved[t * N + e].w) & 0xFFFFu;
            const long back = (long)min(idx, (unsigned)(g.window - 1));
            int src;
            if ((mask >> k) & 1u) src = FWG_GOAL_SRC_DONE;
            else if (g.has_delta && back > t) src = FWG_GOAL_SRC_WINDOW;
            else {
                const u4 b = philox4x32(A.env_base + (unsigned)e, A.serial, (unsigned)t, FWG_STREAM_GOAL, A.seed_lo, A.seed_hi);
                if ((unsigned long long)b.y >= A.p_scaled) src = FWG_GOAL_SRC_KEPT;
                else src = (int)(t + 1 + (long)(((unsigned long long)b.x * (unsigned long long)(R - t)) >> 32));
            }
            float4 goal = src >= 0 ? A.achieved[(long)src * N + e] : A.desired[t * N + e];   // the gather: one 16-byte load per lane
            goal.w = 0.f;
            A.desired_out[t * N + e] = goal;
            A.src_out[t * N + e] = src;
        }
    }
}

// launch 2: one lane per transition, i = t N + e -- the reward of the new goal (read back from desired_out) where launch 1
// relabelled, the raw reward's own bits elsewhere
__global__ __launch_bounds__(256) void k_goal_relabel_reward(const DevCfg* __restrict__ cfg, GoalCfg g, GoalRelabel A) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.T * A.N) return;
    const DevCfg& c = *cfg;
    const long N = A.N, t = i / N;
    float reward = A.raw[i];
    if (A.src_out[i] >= 0) {
        const float4 a0 = A.achieved[i];
        const unsigned idx = __float_as_uint(a0.w) & 0xFFFFu;
        const long back = (long)min(idx, (unsigned)(g.window - 1));
        GoalWin win;
#pragma unroll
        for (int j = 0; j < FWG_MAX_WINDOW; ++j) {
            win.a[j][0] = win.a[j][1] = win.a[j][2] = 0.f;
            if (j <= back && j <= t) {
                const float* p = A.actions + (i - j * N) * 3;
                win.a[j][0] = p[0]; win.a[j][1] = p[1]; win.a[j][2] = p[2];
            }
        }
        reward = goal_reward(c, g, A.achieved[i + N], A.desired_out[i], a0, win, idx);
    }
    A.reward_out[i] = reward;
}

#endif /* FWGYM_GOAL_H */
