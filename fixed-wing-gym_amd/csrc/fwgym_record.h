// fwgym_record.h -- the device flight recorder (fwg_record_start, fwg_record; include/fwgym.h "Flight recorder").
//
// The reference's training callback renders one training episode every few minutes (examples/train_rl_controller.py:31-110:
// env_method("render", indices=0, ...)); its env keeps the episode's history on the host, one append per step.  A rollout here is
// a replayed graph with no host read inside, so the history is kept by a small kernel launched behind every env step: for K
// tracked envs it appends one 32-word row (128 B: one line) to the env's OPEN slab and, at an episode end, flips the env's two
// slabs, so that the last completed episode stays readable while the next one is written.  All recorder state lives in the
// caller's `rows` and `hdr`; nothing travels by value that changes from step to step, so the launches can be captured and replayed.
//
// Shape: one wave per tracked env (grid K, block 64).  Lane w < 32 gathers word w of the appended row, lane 32 + w word w of the
// next episode's row 0 (auto-reset: the arena already holds its reset state when the step that ended the episode returns); each
// row goes out as one 128-B line.  Lane 0 owns the header, which no other block touches.  Every branch is wave-uniform (it depends
// on the block's env and header only).  Plain loads and stores; the one barrier orders the lanes' header reads before lane 0's
// header write (a single wave: it costs nothing, and the host emulation runs its lanes one after the other).
#ifndef FWGYM_RECORD_H
#define FWGYM_RECORD_H

#define FWG_REC_WORDS 32
#define FWG_REC_MAX_TRACKED 64
// hdr[k][8]: word 0 = flags, 1 = rows in the open slab, 2 = rows in the completed slab, 3 = FWG_TERM_* of the completed episode,
// 4 / 5 = episode serial (the arena's episode word) of the open / the completed slab, 6 = episodes completed, 7 = 0
#define FWG_REC_F_SLAB 1          /* index of the open slab */
#define FWG_REC_F_OPEN 2          /* an episode is open */
#define FWG_REC_F_OVERFLOW 4      /* the open episode lost rows past max_rows */
#define FWG_REC_F_OVERFLOW_DONE 8 /* the completed episode did */
#define FWG_REC_F_INVALID 16      /* ids[k] is outside [0, N): the slot records nothing */

// what the recorder needs of the handle's configuration, by value (structure only: none of it changes after fwg_create)
struct RecCfg { int sim, cold, derived, gym, store_derived, turbulence, auto_reset; };

__device__ __forceinline__ float rec_nan() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ float rec_arena(const float* __restrict__ S, long N, long e, int w) { return S[((long)(w >> 2) * N + e) * 4 + (w & 3)]; }

// roll pitch yaw Va alpha beta (i = 0..5) of the committed state: the arena's copy where the step kernel keeps one, else computed
// from the committed quaternion / body velocity and the steady wind as the step kernel computes them (fwgym_physics.h derive)
__device__ __forceinline__ float rec_derived(const RecCfg& rc, const float* __restrict__ S, long N, long e, int i) {
    if (rc.store_derived) return rec_arena(S, N, e, rc.derived + i);
    // (with turbulence the air data depend on the step's gust, which is gone: store_sim keeps alpha beta Va in the second group)
    if (rc.turbulence && i >= 3) return rec_arena(S, N, e, rc.derived + (i == 3 ? 6 : i));
    float y[NY];
#pragma unroll
    for (int j = 0; j < NY; ++j) y[j] = j < 16 ? rec_arena(S, N, e, rc.sim + j) : 0.f;
    const float wind[3] = {rec_arena(S, N, e, rc.cold), rec_arena(S, N, e, rc.cold + 1), rec_arena(S, N, e, rc.cold + 2)};
    Derived d;
    if (rc.turbulence) {
        float ea[5];
        euler_args(y, ea);
        euler_from_args(ea, d);
        d.Va = 0.f; d.alpha = 0.f; d.beta = 0.f;
    } else {
        const float gust[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        d = derive<false>(y, wind, gust);
    }
    return i == 0 ? d.roll : i == 1 ? d.pitch : i == 2 ? d.yaw : i == 3 ? d.Va : i == 4 ? d.alpha : d.beta;
}

// word w of a row of env e.  state: words 0..24 come from the arena (else NaN); step: words 25..28 and 30 come from the step's
// action / reward / done / term_code (else NaN and 0: the row of a reset)
__device__ __forceinline__ float rec_word(const RecCfg& rc, const float* __restrict__ S, long N, long e, int w, bool state, bool step,
                                          const float* __restrict__ actions, const float* __restrict__ reward, unsigned done, unsigned term) {
    if (w < 25) {
        if (!state) return rec_nan();
        if (w < 16) return rec_arena(S, N, e, rc.sim + w);
        if (w < 22) return rec_derived(rc, S, N, e, w - 16);
        return rec_arena(S, N, e, rc.gym + (w - 22));
    }
    if (w < 28) return step ? actions[3 * e + (w - 25)] : rec_nan();
    if (w == 28) return step ? reward[e] : rec_nan();
    if (w == 29) return rec_arena(S, N, e, rc.gym + 3);
    if (w == 30) return __uint_as_float(step ? (done | (term << 8)) : 0u);
    return 0.f;
}

__device__ __forceinline__ float* rec_row(float* rows, int n_tracked, long max_rows, int slab, int k, long r) {
    return rows + (((long)slab * n_tracked + k) * max_rows + r) * FWG_REC_WORDS;
}

// after fwg_reset: every selected tracked env drops the episode in progress (never completed) and starts a new one with row 0
__global__ __launch_bounds__(64) void k_record_start(RecCfg rc, const float* __restrict__ S, long N, const long long* __restrict__ ids, int n_tracked,
                                                     const unsigned char* __restrict__ mask, float* __restrict__ rows, int* __restrict__ hdr, long max_rows) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const long e = (long)ids[k];
    int* H = hdr + 8 * k;
    const int flags = H[0];
    __syncthreads();
    if (e < 0 || e >= N) {
        if (lane == 0) H[0] = flags | FWG_REC_F_INVALID;
        return;
    }
    if (mask != nullptr && mask[e] == 0) return;
    const int slab = flags & FWG_REC_F_SLAB;
    if (lane < FWG_REC_WORDS) rec_row(rows, n_tracked, max_rows, slab, k, 0)[lane] = rec_word(rc, S, N, e, lane, true, false, nullptr, nullptr, 0u, 0u);
    if (lane == 0) {
        H[0] = (flags & ~FWG_REC_F_OVERFLOW) | FWG_REC_F_OPEN;
        H[1] = 1;
        H[4] = (int)__float_as_uint(rec_arena(S, N, e, rc.cold + 3));
    }
}

// after fwg_step, with the action batch it consumed and its reward / done / term_code outputs
__global__ __launch_bounds__(64) void k_record(RecCfg rc, const float* __restrict__ S, long N, const long long* __restrict__ ids, int n_tracked,
                                               const float* __restrict__ actions, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                               const unsigned char* __restrict__ term, float* __restrict__ rows, int* __restrict__ hdr, long max_rows) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const long e = (long)ids[k];
    int* H = hdr + 8 * k;
    const int flags = H[0], n = H[1], serial = H[4], completed = H[6];
    __syncthreads();
    if (e < 0 || e >= N) {
        if (lane == 0) H[0] = flags | FWG_REC_F_INVALID;
        return;
    }
    if (!(flags & FWG_REC_F_OPEN)) return;   // (auto-reset off: a finished env keeps reporting done; only the first end counts)
    const int slab = flags & FWG_REC_F_SLAB;
    const unsigned d = done[e] != 0 ? 1u : 0u, tc = term[e];
    // the terminal sample exists only where the arena still holds it: not after an auto-reset (the arena holds the next episode),
    // not after a simulator failure (the state was not committed; the single-env class records none either)
    const bool state = !d || (!rc.auto_reset && (tc == FWG_TERM_STEPS || tc == FWG_TERM_SUCCESS));
    const bool fits = n >= 0 && n < max_rows;   // (never past a slab, whatever the caller's header holds)
    const bool reopen = d && rc.auto_reset;
    const int w = lane & (FWG_REC_WORDS - 1);
    if (lane < FWG_REC_WORDS) {
        if (fits) rec_row(rows, n_tracked, max_rows, slab, k, n)[w] = rec_word(rc, S, N, e, w, state, true, actions, reward, d, tc);
    } else if (reopen) {
        rec_row(rows, n_tracked, max_rows, slab ^ 1, k, 0)[w] = rec_word(rc, S, N, e, w, true, false, nullptr, nullptr, 0u, 0u);
    }
    if (lane != 0) return;
    int f = flags | (fits ? 0 : FWG_REC_F_OVERFLOW);
    const int n_new = n + (fits ? 1 : 0);
    if (!d) {
        H[0] = f; H[1] = n_new;
        return;
    }
    // the episode ends: its slab becomes the completed one (no copy), the other one the open one
    f = (f & ~FWG_REC_F_OVERFLOW_DONE) | ((f & FWG_REC_F_OVERFLOW) ? FWG_REC_F_OVERFLOW_DONE : 0);
    f = (f & ~(FWG_REC_F_OVERFLOW | FWG_REC_F_OPEN)) ^ FWG_REC_F_SLAB;
    H[2] = n_new; H[3] = (int)tc; H[5] = serial; H[6] = completed + 1;
    if (reopen) {
        f |= FWG_REC_F_OPEN;
        H[1] = 1;
        H[4] = (int)__float_as_uint(rec_arena(S, N, e, rc.cold + 3));
    } else {
        H[1] = 0;
    }
    H[0] = f;
}

#endif /* FWGYM_RECORD_H */
