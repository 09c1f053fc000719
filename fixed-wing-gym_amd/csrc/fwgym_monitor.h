// fwgym_monitor.h -- the device training monitor (fwg_monitor_fold, fwg_monitor_take; include/fwgym.h "Training monitor").
//
// stable-baselines' Monitor wrapper gives every finished episode its undiscounted return `r` and its length `l`, and PPO2 logs
// their means (ep_rewmean / eplenmean) -- what the reference's training callback starts from (examples/train_rl_controller.py
// monitor_training).  A rollout here is a replayed graph with no host read inside and its reward buffer holds VecNormalize'd
// values, so the raw reward of every step is written into a rollout buffer of its own by the step kernel (its reward_out
// argument: no extra launch) and folded ONCE per rollout by k_monitor_fold.
//
// Semantics, per env in step order, over raw_rewards [T][N] and dones [T][N] (the numpy restatement is tests/monitor_common.py):
//   q_t = (int64) rintf(r_t * 2^20)              (FWG_ACC_SCALE; the product is exact in float, the rounding is to nearest even)
//   a reward is BAD when !(fabsf(r_t) <= 2^20)   (NaN, inf, anything the bound below excludes)
//   good reward: ep_q += q_t;   bad reward: bit 31 of ep_len is set;   either way ep_len += 1
//   dones[t][e] != 0: the episode is emitted WITH the reward of step t and the carry (ep_q, ep_len) goes to zero.
//     a flagged episode (bit 31) adds 1 to `nonfinite` and nothing else; any other one updates episodes, sum_q, sum_len,
//     min_q, max_q, min_len, max_len
// ep_q_io / ep_len_io carry the open episode from one fold to the next.  Bounds: |r| <= 2^20 per step and steps_max < 65 535, so
// |ep_q| < 2^56 and the low 31 bits of ep_len never reach bit 31.
// Everything summed is an integer, so the fold is exactly associative: the result does not depend on how the kernel splits time,
// on the order of the waves, or on how the envs are sharded over ranks.  The price is the quantisation, at most 2^-21 per step.
//
// Shape (k_gae's): a workgroup of four waves takes 64 adjacent envs x a span of 128 steps, wave w the segment [w L, (w + 1) L) of
// it, L = 32.  Every lane requests its 32 rewards and 32 done flags at once (step-major: a wave reads 256-B reward rows and 64-B
// done rows), then scans them in registers.  A segment summarises to: has_done; the head (q, len | bad) up to and including its
// first done (the whole segment when it has none); the tail after its last done; and the episodes that lie wholly inside it,
// which the lane adds to its own aggregates at once.  The heads and tails go through LDS; after ONE barrier wave 0 merges them
// left to right into the carry it holds in registers and emits the episodes that cross a segment boundary.  Longer rollouts
// are walked in spans.  At the end the lanes' aggregates are reduced over the wave by shuffles and over the four waves through
// LDS, and thread 0 read-modify-writes the workgroup's OWN slot of `scratch` ([blocks][8] 64-bit words, blocks = ceil(N / 64))
// with plain loads and stores: no atomics, launches are stream-ordered.  An all-zero slot is the identity (the min / max words
// of a slot count only where its episodes word is non-zero), so a zeroed scratch is ready for the first fold.
// Lanes with e >= N load env N - 1's values (no out-of-bounds address) and contribute nothing.
#ifndef FWGYM_MONITOR_H
#define FWGYM_MONITOR_H

#ifndef FWG_N_MONITOR
#define FWG_N_MONITOR 8   /* include/fwgym.h */
#endif
#define FWG_MON_L 32                      /* steps per wave segment */
#define FWG_MON_SPAN (4 * FWG_MON_L)      /* steps per workgroup span */
#define FWG_MON_BAD 0x80000000u           /* bit 31 of ep_len: the episode holds a bad reward */
#define FWG_MON_LMAX 0x7fffffffffffffffLL
#define FWG_MON_LMIN (-0x7fffffffffffffffLL - 1)
// aggregate words: 0 episodes, 1 nonfinite, 2 sum_q, 3 sum_len, 4 min_q, 5 max_q, 6 min_len, 7 max_len

__device__ __forceinline__ void mon_identity(long long (&a)[FWG_N_MONITOR]) {
    a[0] = a[1] = a[2] = a[3] = 0;
    a[4] = a[6] = FWG_MON_LMAX;
    a[5] = a[7] = FWG_MON_LMIN;
}
// a += b, word by word: sums, minima, maxima
__device__ __forceinline__ void mon_combine(long long (&a)[FWG_N_MONITOR], const long long (&b)[FWG_N_MONITOR]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] += b[i];
    a[4] = b[4] < a[4] ? b[4] : a[4];
    a[5] = b[5] > a[5] ? b[5] : a[5];
    a[6] = b[6] < a[6] ? b[6] : a[6];
    a[7] = b[7] > a[7] ? b[7] : a[7];
}
// one finished episode into a lane's aggregates
__device__ __forceinline__ void mon_emit(long long (&a)[FWG_N_MONITOR], long long q, unsigned len) {
    if (len & FWG_MON_BAD) { a[1] += 1; return; }
    const long long l = (long long)len;
    a[0] += 1; a[2] += q; a[3] += l;
    a[4] = q < a[4] ? q : a[4];
    a[5] = q > a[5] ? q : a[5];
    a[6] = l < a[6] ? l : a[6];
    a[7] = l > a[7] ? l : a[7];
}
// two pieces of one episode: the lengths add, the bad flags OR
__device__ __forceinline__ unsigned mon_join_len(unsigned a, unsigned b) {
    return ((a & ~FWG_MON_BAD) + (b & ~FWG_MON_BAD)) | ((a | b) & FWG_MON_BAD);
}
// 64-bit value of lane (l ^ mask): two 32-bit shuffles (bit moves; the host emulation has the float form only)
__device__ __forceinline__ long long mon_xor64(long long v, int mask) {
    const unsigned long long u = (unsigned long long)v;
    const unsigned lo = __float_as_uint(__shfl_xor(__uint_as_float((unsigned)u), mask, FWG_WAVE));
    const unsigned hi = __float_as_uint(__shfl_xor(__uint_as_float((unsigned)(u >> 32)), mask, FWG_WAVE));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// the 256 lanes' aggregates -> thread 0's `a` (red: LDS, [4 waves][8] 64-bit words, free to overwrite)
__device__ __forceinline__ void mon_block_reduce(long long (&a)[FWG_N_MONITOR], long long* red, int lane, int w) {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
        long long b[FWG_N_MONITOR];
#pragma unroll
        for (int i = 0; i < FWG_N_MONITOR; ++i) b[i] = mon_xor64(a[i], mask);
        mon_combine(a, b);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < FWG_N_MONITOR; ++i) red[w * FWG_N_MONITOR + i] = a[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            long long b[FWG_N_MONITOR];
#pragma unroll
            for (int i = 0; i < FWG_N_MONITOR; ++i) b[i] = red[j * FWG_N_MONITOR + i];
            mon_combine(a, b);
        }
    }
}

__global__ __launch_bounds__(256) void k_monitor_fold(const float* __restrict__ rew, const unsigned char* __restrict__ done,
                                                      long long* __restrict__ ep_q, int* __restrict__ ep_len,
                                                      long long* __restrict__ scratch, long T, long N) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    long long* const seg = reinterpret_cast<long long*>(lds);   // [4 waves][4 words][64 lanes]: head q, tail q, head len | tail len << 32, has_done
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long e0 = (long)blockIdx.x * 64 + lane;
    const bool valid = e0 < N;
    const long e = valid ? e0 : N - 1;
    long long a[FWG_N_MONITOR];
    mon_identity(a);
    long long cq = 0;                                           // the open episode (wave 0 carries it from span to span)
    unsigned cl = 0;
    if (w == 0 && valid) { cq = ep_q[e]; cl = (unsigned)ep_len[e]; }
    for (long lo = 0; lo < T; lo += FWG_MON_SPAN) {
        const long hi = lo + FWG_MON_SPAN < T ? lo + FWG_MON_SPAN : T;
        const long s0 = lo + (long)w * FWG_MON_L;               // this wave's segment [s0, s1) (empty past the end of a short span)
        const long s1 = s0 + FWG_MON_L < hi ? s0 + FWG_MON_L : hi;
        float r[FWG_MON_L];
        unsigned char d[FWG_MON_L];
#pragma unroll
        for (int k = 0; k < FWG_MON_L; ++k) {
            const long t = s0 + k;
            if (t < s1) { r[k] = rew[t * N + e]; d[k] = done[t * N + e]; }
        }
        long long q = 0, hq = 0;
        unsigned len = 0, hl = 0;
        bool seen = false;
#pragma unroll
        for (int k = 0; k < FWG_MON_L; ++k) {
            if (s0 + k < s1) {
                const float x = r[k];
                const bool good = fabsf(x) <= FWG_ACC_SCALE;
                const long long qk = good ? (long long)rintf(x * FWG_ACC_SCALE) : 0;
                q += qk;
                len = (len + 1) | (good ? 0u : FWG_MON_BAD);
                if (d[k] && valid) {
                    if (!seen) { hq = q; hl = len; seen = true; }
                    else mon_emit(a, q, len);
                    q = 0; len = 0;
                }
            }
        }
        if (!seen) { hq = q; hl = len; q = 0; len = 0; }         // no done: the whole segment is the head (an empty one the identity)
        seg[(w * 4 + 0) * 64 + lane] = hq;
        seg[(w * 4 + 1) * 64 + lane] = q;
        seg[(w * 4 + 2) * 64 + lane] = (long long)((unsigned long long)hl | ((unsigned long long)len << 32));
        seg[(w * 4 + 3) * 64 + lane] = seen ? 1 : 0;
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long lens = (unsigned long long)seg[(j * 4 + 2) * 64 + lane];
                cq += seg[(j * 4 + 0) * 64 + lane];
                cl = mon_join_len(cl, (unsigned)lens);
                if (seg[(j * 4 + 3) * 64 + lane] != 0) {
                    mon_emit(a, cq, cl);
                    cq = seg[(j * 4 + 1) * 64 + lane];
                    cl = (unsigned)(lens >> 32);
                }
            }
        }
        __syncthreads();                                         // the summaries are read before the next span (or the reduction) overwrites them
    }
    if (w == 0 && valid) { ep_q[e] = cq; ep_len[e] = (int)cl; }
    mon_block_reduce(a, seg, lane, w);
    if (threadIdx.x == 0 && (a[0] | a[1]) != 0) {
        long long* const s = scratch + (long)blockIdx.x * FWG_N_MONITOR;
        long long old[FWG_N_MONITOR];
#pragma unroll
        for (int i = 0; i < FWG_N_MONITOR; ++i) old[i] = s[i];
        if (old[0] == 0) { old[4] = old[6] = FWG_MON_LMAX; old[5] = old[7] = FWG_MON_LMIN; }
        mon_combine(old, a);
        if (old[0] == 0) old[4] = old[5] = old[6] = old[7] = 0;  // (only flagged episodes so far: the slot's min / max words stay zero)
#pragma unroll
        for (int i = 0; i < FWG_N_MONITOR; ++i) s[i] = old[i];
    }
}

// one workgroup: the slots in index order (thread i takes slots i, i + 256, ...), cleared as they are read; then the 8 doubles
__global__ __launch_bounds__(256) void k_monitor_take(long long* __restrict__ scratch, double* __restrict__ out, long blocks) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    long long* const red = reinterpret_cast<long long*>(lds);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long a[FWG_N_MONITOR];
    mon_identity(a);
    for (long b = threadIdx.x; b < blocks; b += 256) {
        long long* const s = scratch + b * FWG_N_MONITOR;
        long long v[FWG_N_MONITOR];
#pragma unroll
        for (int i = 0; i < FWG_N_MONITOR; ++i) { v[i] = s[i]; s[i] = 0; }
        if (v[0] == 0) { v[4] = v[6] = FWG_MON_LMAX; v[5] = v[7] = FWG_MON_LMIN; }
        mon_combine(a, v);
    }
    mon_block_reduce(a, red, lane, w);
    if (threadIdx.x == 0) {
        const double inv = 1.0 / (double)FWG_ACC_SCALE, inf = (double)INFINITY;
        const bool any = a[0] != 0;
        out[0] = (double)a[0];
        out[1] = (double)a[1];
        out[2] = (double)a[2] * inv;
        out[3] = (double)a[3];
        out[4] = any ? (double)a[4] * inv : inf;
        out[5] = any ? (double)a[5] * inv : -inf;
        out[6] = any ? (double)a[6] : inf;
        out[7] = any ? (double)a[7] : -inf;
    }
}

#endif
