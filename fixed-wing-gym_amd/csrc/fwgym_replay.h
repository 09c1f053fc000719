// fwgym_replay.h -- a hindsight replay buffer on the device: the episode index of a stored rollout and minibatches relabelled while
// they are drawn (fwg_replay_index, fwg_replay_sample; include/fwgym.h "Hindsight replay").
//
// fwg_goal_relabel (fwgym_goal.h) relabels ONE rollout once, in place and in rollout order.  An off-policy learner keeps many
// rollouts ("slots") on the device, draws minibatches uniformly over all of them and wants a fresh hindsight goal -- with that
// goal's reward -- every time a transition is drawn.  Two stateless launches over caller-owned buffers do that; their semantics are
// normative in include/fwgym.h and restated in numpy by tests/replay_common.py.
//
// k_replay_index: ep_end[t][n] = the first t_e > t with a done in column n, or T -- the R of k_goal_relabel, whose span / segment
// scan it is (four waves x 64 adjacent envs x a span of 128 steps, one barrier pair per span), without the draw.  It runs once per
// stored rollout, so that a sample costs one 4-byte load where a forward scan would walk byte loads N apart.
//
// k_replay_sample: a workgroup of 256 lanes takes 256 samples, in two phases around one barrier.
//   1  one lane per sample: the Philox draw of (slot, step, env), the decision src, the gather of the goal rows and of the action
//      window, the reward function (goal_reward of fwgym_goal.h, as k_goal_relabel_reward calls it) and the small outputs.  Every
//      load is a random address, one line each: the lane's 256 samples keep that many lines in flight.  The lane leaves the row
//      number of its observation in LDS (8 bytes per sample).
//   2  the two observation rows of a sample are 4 D bytes from a random address: consecutive lanes take consecutive 16-byte pieces
//      (D % 4 == 0) or words (any other D) of the same row, so that a row is fetched by adjacent lanes in one or two requests and
//      the output rows, which are adjacent in memory, are written coalesced.
// No atomics, no scratch, no spills; nothing is read outside the slot the sample fell into.
#ifndef FWGYM_REPLAY_H
#define FWGYM_REPLAY_H

#define FWG_STREAM_REPLAY 11u             /* Philox stream of the replay draws (1..10 are taken, fwgym_dev.h / fwgym_actor.h / fwgym_goal.h) */
#define FWG_REPLAY_BLOCK 256              /* samples per workgroup */

// one launch per stored rollout: dones [T][N] -> ep_end [T][N]
__global__ __launch_bounds__(256) void k_replay_index(long T, long N, const unsigned char* __restrict__ done, int* __restrict__ ep_end) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int* const first = reinterpret_cast<int*>(lds);   // [4 waves][64 lanes]: step of the segment's first done, or -1
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long e0 = (long)blockIdx.x * 64 + lane;
    const bool valid = e0 < N;
    const long e = valid ? e0 : N - 1;   // (lanes past the last env load its values and store nothing)
    long carry = T;   // the first done of the spans after this one, or T
    for (long lo = ((T - 1) / FWG_GOAL_SPAN) * FWG_GOAL_SPAN; lo >= 0; lo -= FWG_GOAL_SPAN) {
        const long hi = lo + FWG_GOAL_SPAN < T ? lo + FWG_GOAL_SPAN : T;
        const long s0 = lo + (long)w * FWG_GOAL_L;   // this wave's segment [s0, s1) (empty past the end of a short span)
        const long s1 = s0 + FWG_GOAL_L < hi ? s0 + FWG_GOAL_L : hi;
        unsigned mask = 0u;
#pragma unroll
        for (int k = 0; k < FWG_GOAL_L; ++k)
            if (s0 + k < s1) mask |= done[(s0 + k) * N + e] != 0 ? (1u << k) : 0u;
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
            ep_end[t * N + e] = (int)(later != 0u ? t + __ffsll((long long)later) : after);
        }
    }
}

struct ReplaySample {
    const float* obs;             // [K][T + 1][N][D]
    const float* actions;         // [K][T][N][3]
    const float* raw;             // [K][T][N]
    const unsigned char* done;    // [K][T][N]
    const int* ep_end;            // [K][T][N]
    const float4* achieved;       // [K][T + 1][N]
    const float4* desired;        // [K][T + 1][N]
    float* obs_out;               // [B][D]
    float* next_obs_out;          // [B][D]
    float* action_out;            // [B][3]
    float4* achieved_out;         // [B]
    float4* desired_out;          // [B]
    float* reward_out;            // [B]
    unsigned char* done_out;      // [B]
    int* index_out;               // [B][4]
    long T, N, B;
    int D, strategy, vec4;        // vec4: D % 4 == 0 and the three observation buffers are 16-byte aligned
    unsigned n_slots, n_filled, serial, seed_lo, seed_hi;
    unsigned long long p_scaled;
};
struct alignas(16) ReplayIdx { int k, t, n, src; };

__global__ __launch_bounds__(FWG_REPLAY_BLOCK) void k_replay_sample(const DevCfg* __restrict__ cfg, GoalCfg g, ReplaySample A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    long* const row_of = reinterpret_cast<long*>(lds);   // [256]: (k (T + 1) + t) N + n of the block's samples
    const long base = (long)blockIdx.x * FWG_REPLAY_BLOCK;
    const long i = base + threadIdx.x;
    const long T = A.T, N = A.N;
    // ---- phase 1: one lane per sample
    if (i < A.B) {
        const DevCfg& c = *cfg;
        const u4 a = philox4x32((unsigned)i, A.serial, 0u, FWG_STREAM_REPLAY, A.seed_lo, A.seed_hi);
        const long k = (long)__umulhi(a.x, A.n_filled);
        const long t = (long)__umulhi(a.y, (unsigned)T);
        const long n = (long)__umulhi(a.z, (unsigned)N);
        const long tr = (k * T + t) * N + n;         // the transition in the [K][T][N] buffers
        const long row = (k * (T + 1) + t) * N + n;  // its row in the [K][T + 1][N] buffers (the row behind it: row + N)
        const float4* const ach = A.achieved + k * (T + 1) * N + n;   // the goal rows of the sample's slot and env: row r at ach[r N]
        const float4 a0 = A.achieved[row];
        const unsigned char dn = A.done[tr];
        long R = (long)A.ep_end[tr];
        R = R > T ? T : (R <= t ? t + 1 : R);        // (fwg_replay_index gives t < R <= T: nothing is read outside the slot whatever the buffer holds)
        const unsigned idx = __float_as_uint(a0.w) & 0xFFFFu;
        const long back = (long)min(idx, (unsigned)(g.window - 1));
        int src;
        if (dn != 0) src = FWG_GOAL_SRC_DONE;
        else if (g.has_delta && back > t) src = FWG_GOAL_SRC_WINDOW;
        else if ((unsigned long long)a.w >= A.p_scaled) src = FWG_GOAL_SRC_KEPT;
        else if (A.strategy == FWG_REPLAY_FINAL) src = (int)R;
        else {
            const u4 b = philox4x32((unsigned)i, A.serial, 1u, FWG_STREAM_REPLAY, A.seed_lo, A.seed_hi);
            const long s0 = A.strategy == FWG_REPLAY_EPISODE ? (t > (long)idx ? t - (long)idx : 0) : t;
            src = (int)(s0 + 1 + (long)__umulhi(b.x, (unsigned)(R - s0)));
        }
        const float4 a1 = A.achieved[row + N];
        float4 goal = src >= 0 ? ach[(long)src * N] : A.desired[row];
        goal.w = 0.f;
        const float* const act = A.actions + tr * 3;
        float reward = A.raw[tr];
        if (src >= 0) {
            GoalWin win;
#pragma unroll
            for (int j = 0; j < FWG_MAX_WINDOW; ++j) {
                win.a[j][0] = win.a[j][1] = win.a[j][2] = 0.f;
                if (j <= back && j <= t) {
                    const float* p = act - (long)j * N * 3;
                    win.a[j][0] = p[0]; win.a[j][1] = p[1]; win.a[j][2] = p[2];
                }
            }
            reward = goal_reward(c, g, a1, goal, a0, win, idx);
        }
        A.action_out[i * 3] = act[0]; A.action_out[i * 3 + 1] = act[1]; A.action_out[i * 3 + 2] = act[2];
        A.achieved_out[i] = make_float4(a1.x, a1.y, a1.z, 0.f);
        A.desired_out[i] = goal;
        A.reward_out[i] = reward;
        A.done_out[i] = dn;
        *reinterpret_cast<ReplayIdx*>(A.index_out + i * 4) = ReplayIdx{(int)k, (int)t, (int)n, src};
        row_of[threadIdx.x] = row;
    }
    __syncthreads();
    // ---- phase 2: the observation rows, adjacent lanes on adjacent pieces of one row
    const long left = A.B - base;
    const int ns = left < FWG_REPLAY_BLOCK ? (int)left : FWG_REPLAY_BLOCK;
    if (A.vec4) {
        const int Q = A.D >> 2, per = 2 * Q;   // 16-byte pieces per row / per sample
        for (int item = threadIdx.x; item < ns * per; item += FWG_REPLAY_BLOCK) {
            const int s = item / per, rem = item - s * per;
            const int nxt = rem >= Q ? 1 : 0, q = rem - nxt * Q;
            const float4 v = reinterpret_cast<const float4*>(A.obs + (row_of[s] + nxt * N) * A.D)[q];
            reinterpret_cast<float4*>((nxt ? A.next_obs_out : A.obs_out) + (base + s) * A.D)[q] = v;
        }
    } else {
        const int per = 2 * A.D;
        for (int item = threadIdx.x; item < ns * per; item += FWG_REPLAY_BLOCK) {
            const int s = item / per, rem = item - s * per;
            const int nxt = rem >= A.D ? 1 : 0, q = rem - nxt * A.D;
            (nxt ? A.next_obs_out : A.obs_out)[(base + s) * A.D + q] = A.obs[(row_of[s] + nxt * N) * A.D + q];
        }
    }
}

#endif /* FWGYM_REPLAY_H */
