// fwgym_offpolicy.h -- the off-policy update on the device (include/fwgym.h "Off-policy update"): DDPG, or TD3's clipped double-Q
// and delayed actor step, on minibatches as replay.HindsightReplay.sample returns them.  The scheme is the PPO update's
// (fwgym_learner.h): 64-row tiles in LDS, every GEMM on v_mfma_f32_32x32x16_bf16 with fp32 operands split hi + lo (ppo_mma_tile),
// one partial-gradient slab per workgroup, the slabs summed in a fixed order (no float atomics: bitwise deterministic), a
// one-workgroup Adam.  Five kernels:
//   k_ddpg_critic_grad : per tile -- a' = pi_target(o', g), q' = min_j Q_target,j(o', g, a'), y = r + gamma (1 - done) q', then every
//                        critic's forward and backward on (o, g, a); slab = the critics' gradients, sum (Q - y)^2, sum Q_0, sum y
//   k_ddpg_actor_grad  : per tile -- pi(o, g), Q_0(o, g, pi), back through the critic for dQ / da only, through tanh and the actor;
//                        slab = the actor's gradients and sum Q
//   k_ddpg_reduce      : one segment of the flat gradient (the actor's, or the critics') and its loss sums from the slabs
//   k_ddpg_apply       : Adam (torch's form, eps 1e-8 by default) on that segment, optional clip_grad_norm_, the statistics
//   k_ddpg_polyak      : theta_t <- lerp(theta_t, theta, tau) over the whole vector (torch's lerp_: exact at tau = 0 and tau = 1)
// Hidden layers 64-64 with ReLU (stable-baselines' DDPG / TD3 default); online and target parameters are two flat fp32 vectors
// with one layout, actor.parameters() | critic0.parameters() | critic1.parameters() of nn.Sequential(Linear, ReLU, Linear, ReLU,
// Linear[, Tanh]):  W1 [64][K] b1 [64] W2 [64][64] b2 [64] W3 [nout][64] b3 [nout],  K = D + G (actor), D + G + A (critics).
// A gradient vector has the same layout and FWG_DDPG_NSTAT loss sums behind it.
#pragma once
#include "fwgym_learner.h"

#define FWG_DDPG_NSTAT 4           // loss sums behind a gradient: sum (Q_j - y)^2 over j, sum Q_0(o,g,pi) [actor launch], sum Q_0(o,g,a), sum y
#define FWG_DDPG_GOAL_STRIDE 4     // words per goal row (replay.sample's desired_rows)
#define FWG_DDPG_TILES_CRITIC 5
#define FWG_DDPG_TILES_ACTOR 6

struct DdpgNet { int w1, b1, w2, b2, w3, b3; };
// D observation words, G goal words, A actions, NC critics; Ka / Kc the input widths; PA the actor's parameters (= where the
// critics' segment starts), P all of them, SW floats per slab
struct DdpgLayout { int D, G, A, NC, Ka, Kc, PA, P, SW; DdpgNet actor, critic[2]; };
// (double, as PpoHparams: torch computes Adam's scalars from doubles).  max_norm_* <= 0: no clipping
struct DdpgHparams { double gamma, tau, lr_actor, lr_critic, beta1, beta2, eps, max_norm_actor, max_norm_critic; };
struct DdpgBatch { const float *obs, *next_obs, *act, *goal, *rew; const unsigned char* done; };

__host__ __device__ inline int ddpg_net_layout(DdpgNet& N, int o, int K, int nout) {
    N.w1 = o; o += 64 * K;
    N.b1 = o; o += 64;
    N.w2 = o; o += 64 * 64;
    N.b2 = o; o += 64;
    N.w3 = o; o += nout * 64;
    N.b3 = o; o += nout;
    return o;
}
__host__ __device__ inline DdpgLayout ddpg_layout(int D, int G, int A, int NC) {
    DdpgLayout L;
    L.D = D; L.G = G; L.A = A; L.NC = NC; L.Ka = D + G; L.Kc = D + G + A;
    int o = ddpg_net_layout(L.actor, 0, L.Ka, A);
    L.PA = o;
    o = ddpg_net_layout(L.critic[0], o, L.Kc, 1);
    L.critic[1] = L.critic[0];
    if (NC > 1) o = ddpg_net_layout(L.critic[1], o, L.Kc, 1);
    L.P = o;
    L.SW = (o + FWG_DDPG_NSTAT + 3) & ~3;
    return L;
}
__host__ __device__ inline int ddpg_lds_floats(int tiles) { return tiles * FWG_PPO_ROWS * FWG_PPO_LS + 4 * FWG_PPO_ROWS + 8 * FWG_PPO_ROWS; }

// the tile's input rows: [obs | goal | action] (action columns only when `act` is given), 0 beyond and on rows past the batch;
// four threads per row, 16 columns each
__device__ __forceinline__ void ddpg_gather(float* Xs, const DdpgLayout& L, const float* obs, const float* goal, const float* act, long r0,
                                            int nrows, int tid) {
    const int r = tid >> 2, q = tid & 3;
    const bool ok = r < nrows;
    const long row = ok ? r0 + r : 0;
    for (int f = 16 * q; f < 16 * q + 16; ++f) {
        float v = 0.f;
        if (ok) {
            if (f < L.D) v = obs[row * L.D + f];
            else if (f < L.Ka) v = goal[row * FWG_DDPG_GOAL_STRIDE + f - L.D];
            else if (act != nullptr && f < L.Kc) v = act[row * L.A + f - L.Ka];
        }
        Xs[r * FWG_PPO_LS + f] = v;
    }
}

// one network forward on the tile X [64][LS] of width K: H1 = relu(X W1^T + b1), H2 = relu(H1 W2^T + b2), out [64][4] = H2 W3^T + b3
// (tanh of it for the actor).  Ends behind a barrier
template <bool TANH>
__device__ __forceinline__ void ddpg_forward(const float* P, const DdpgNet& N, int K, int nout, const float* X, float* H1, float* H2, float* out,
                                             int tid) {
    constexpr int LS = FWG_PPO_LS;
    const int l = tid & 63, wv = tid >> 6, half = l >> 5, tm0 = 32 * (wv & 1), tn0 = 32 * (wv >> 1), n = tn0 + (l & 31);
    {
        f32x16 acc = {0.f};
        ppo_mma_tile<true>(acc, X, LS, 1, tm0, 64, P + N.w1, 1, K, tn0, 64, 16 * ((K + 15) / 16), K, l);
        const float bn = P[N.b1 + n];
#pragma unroll
        for (int r = 0; r < 16; ++r) H1[(tm0 + ppo_acc_row(r, half)) * LS + n] = fmaxf(acc[r] + bn, 0.f);
    }
    __syncthreads();
    {
        f32x16 acc = {0.f};
        ppo_mma_tile<true>(acc, H1, LS, 1, tm0, 64, P + N.w2, 1, 64, tn0, 64, 64, 64, l);
        const float bn = P[N.b2 + n];
#pragma unroll
        for (int r = 0; r < 16; ++r) H2[(tm0 + ppo_acc_row(r, half)) * LS + n] = fmaxf(acc[r] + bn, 0.f);
    }
    __syncthreads();
    if (wv < nout) {   // output layer (<= 4 columns: VALU), column wv of row l
        const float* W3 = P + N.w3 + wv * 64;
        float o = P[N.b3 + wv];
#pragma unroll 8
        for (int k = 0; k < 64; ++k) o += H2[l * LS + k] * W3[k];
        out[l * 4 + wv] = TANH ? ppo_tanh(o) : o;
    }
    __syncthreads();
}

// gradient accumulators of one network, kept in registers over a workgroup's tiles
struct DdpgAcc { f32x16 w1, w2; float w3, b3, b2, b1; };
__device__ __forceinline__ void ddpg_acc_zero(DdpgAcc& g) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { g.w1[r] = 0.f; g.w2[r] = 0.f; }
    g.w3 = g.b3 = g.b2 = g.b1 = 0.f;
}

// back through one network from dO [64][4] = dL / d(output before any tanh): G2 = (dO W3) [H2 > 0] into Gb, G1 = (G2 W2) [H1 > 0]
// into Tb (Tb may be H2's tile: H2 is last read before the first barrier).  WG: the weight gradients too (contractions over the
// tile's rows, added to `g`); without it only the input-side gradient G1 is formed.  Ends behind a barrier
template <bool WG>
__device__ __forceinline__ void ddpg_backward(const float* P, const DdpgNet& N, int K, int nout, const float* X, const float* H1, const float* H2,
                                              float* Gb, float* Tb, const float* dO, DdpgAcc& g, int tid) {
    constexpr int LS = FWG_PPO_LS;
    const int l = tid & 63, wv = tid >> 6, half = l >> 5, tm0 = 32 * (wv & 1), tn0 = 32 * (wv >> 1), n = tn0 + (l & 31);
    const float *W2 = P + N.w2, *W3 = P + N.w3;
    if (WG && wv < nout) {
        float s = 0.f, sb = 0.f;
#pragma unroll 8
        for (int r = 0; r < FWG_PPO_ROWS; ++r) { s += dO[r * 4 + wv] * H2[r * LS + l]; sb += dO[r * 4 + wv]; }
        g.w3 += s;
        if (l == 0) g.b3 += sb;
    }
#pragma unroll 4
    for (int j = 0; j < FWG_PPO_ROWS * 64 / FWG_PPO_THREADS; ++j) {
        const int e = tid + FWG_PPO_THREADS * j, r = e >> 6, k = e & 63;
        float s = 0.f;
        for (int o = 0; o < nout; ++o) s += dO[r * 4 + o] * W3[o * 64 + k];
        Gb[r * LS + k] = H2[r * LS + k] > 0.f ? s : 0.f;
    }
    __syncthreads();
    {
        f32x16 acc = {0.f};
        ppo_mma_tile<true>(acc, Gb, LS, 1, tm0, 64, W2, 64, 1, tn0, 64, 64, 64, l);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = tm0 + ppo_acc_row(r, half);
            Tb[m * LS + n] = H1[m * LS + n] > 0.f ? acc[r] : 0.f;
        }
        if (WG) {
            ppo_mma_tile<true>(g.w2, Gb, 1, LS, tm0, 64, H1, LS, 1, tn0, 64, 64, 64, l);
            if (tid < 64) {
                float s = 0.f;
#pragma unroll 8
                for (int r = 0; r < FWG_PPO_ROWS; ++r) s += Gb[r * LS + tid];
                g.b2 += s;
            }
        }
    }
    __syncthreads();
    if (WG) {
        if (tn0 < K) ppo_mma_tile<true>(g.w1, Tb, 1, LS, tm0, 64, X, LS, 1, tn0, K, 64, 64, l);
        if (tid < 64) {
            float s = 0.f;
#pragma unroll 8
            for (int r = 0; r < FWG_PPO_ROWS; ++r) s += Tb[r * LS + tid];
            g.b1 += s;
        }
        __syncthreads();
    }
}

// one network's accumulators into the workgroup's slab: every entry written by exactly one lane
__device__ __forceinline__ void ddpg_store(float* S, const DdpgNet& N, int K, int nout, const DdpgAcc& g, int tid) {
    const int l = tid & 63, wv = tid >> 6, half = l >> 5, tm0 = 32 * (wv & 1), tn0 = 32 * (wv >> 1), n = tn0 + (l & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = tm0 + ppo_acc_row(r, half);
        if (n < K) S[N.w1 + m * K + n] = g.w1[r];
        S[N.w2 + m * 64 + n] = g.w2[r];
    }
    if (wv < nout) {
        S[N.w3 + wv * 64 + l] = g.w3;
        if (l == 0) S[N.b3 + wv] = g.b3;
    }
    if (tid < 64) { S[N.b1 + tid] = g.b1; S[N.b2 + tid] = g.b2; }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ddpg_critic_grad
// ---------------------------------------------------------------------------------------------------------------------
struct DdpgGradArgs {
    DdpgBatch B;
    long n;                 // rows of the batch
    long ntiles;            // ceil(n / 64), spread evenly over gridDim.x workgroups
    const float* params;    // online
    const float* target;    // target (critic launch only)
    float gamma;
    float* slab;            // [gridDim.x][SW]
    float* y_out;           // (critic launch, may be null) [n] the TD targets
    DdpgLayout L;
};

__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ddpg_critic_grad(const DdpgGradArgs G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LS = FWG_PPO_LS;
    const int tid = threadIdx.x;
    const DdpgLayout& L = G.L;
    float* Xs = lds;                        // [64][LS] [o' | g | a'], then [o | g | a]
    float* H1 = Xs + FWG_PPO_ROWS * LS;     // [64][LS] hidden layers of the network in flight (target pass and critic pass)
    float* H2 = H1 + FWG_PPO_ROWS * LS;
    float* Gb = H2 + FWG_PPO_ROWS * LS;     // [64][LS] dL / d(pre-activation 2)
    float* Tb = Gb + FWG_PPO_ROWS * LS;     // [64][LS] dL / d(pre-activation 1)
    float* dO = Tb + FWG_PPO_ROWS * LS;     // [64][4] network outputs, then dL / d(output)
    float* rowf = dO + 4 * FWG_PPO_ROWS;    // [64][8] 0 reward, 1 1 - done, 2 min_j Q_target,j, 3 y; at the end the reduction space
    const float inv_n = 1.f / (float)G.n;
    const long t0 = (long)blockIdx.x * G.ntiles / gridDim.x, t1 = (long)(blockIdx.x + 1) * G.ntiles / gridDim.x;
    DdpgAcc g[2];
    ddpg_acc_zero(g[0]);
    ddpg_acc_zero(g[1]);
    float st[3] = {0.f, 0.f, 0.f};   // sum (Q - y)^2, sum Q_0, sum y over this lane's rows
    for (long t = t0; t < t1; ++t) {
        const long r0 = t * FWG_PPO_ROWS;
        const int nrows = (int)(G.n - r0 < FWG_PPO_ROWS ? G.n - r0 : FWG_PPO_ROWS);
        const bool ok = tid < nrows;
        // ---- the TD target: [o' | g] through the target actor, [o' | g | a'] through the target critics
        ddpg_gather(Xs, L, G.B.next_obs, G.B.goal, nullptr, r0, nrows, tid);
        if (tid < FWG_PPO_ROWS) {
            rowf[tid * 8 + 0] = ok ? G.B.rew[r0 + tid] : 0.f;
            rowf[tid * 8 + 1] = ok ? (G.B.done[r0 + tid] ? 0.f : 1.f) : 0.f;
        }
        __syncthreads();
        ddpg_forward<true>(G.target, L.actor, L.Ka, L.A, Xs, H1, H2, dO, tid);
        if (tid < FWG_PPO_ROWS)
            for (int a = 0; a < L.A; ++a) Xs[tid * LS + L.Ka + a] = dO[tid * 4 + a];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j < L.NC) {
                ddpg_forward<false>(G.target, L.critic[j], L.Kc, 1, Xs, H1, H2, dO, tid);
                if (tid < FWG_PPO_ROWS) rowf[tid * 8 + 2] = j ? fminf(rowf[tid * 8 + 2], dO[tid * 4]) : dO[tid * 4];
            }
        }
        if (tid < FWG_PPO_ROWS) {   // y = r + gamma (1 - done) q': r itself on a terminal row and at gamma = 0
            const float y = rowf[tid * 8 + 0] + G.gamma * (rowf[tid * 8 + 1] * rowf[tid * 8 + 2]);
            rowf[tid * 8 + 3] = y;
            if (ok) {
                st[2] += y;
                if (G.y_out != nullptr) G.y_out[r0 + tid] = y;
            }
        }
        // ---- the critics on [o | g | a] (the forward passes above ended behind a barrier: nobody reads Xs any more)
        ddpg_gather(Xs, L, G.B.obs, G.B.goal, G.B.act, r0, nrows, tid);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // (unrolled: each critic's accumulators stay in registers)
            if (j < L.NC) {
                ddpg_forward<false>(G.params, L.critic[j], L.Kc, 1, Xs, H1, H2, dO, tid);
                if (tid < FWG_PPO_ROWS) {   // L_c = sum_j mean (Q_j - y)^2; rows past the batch contribute nothing
                    const float q = dO[tid * 4], d = q - rowf[tid * 8 + 3];
                    dO[tid * 4] = ok ? 2.f * d * inv_n : 0.f;
                    if (ok) {
                        st[0] += d * d;
                        if (j == 0) st[1] += q;
                    }
                }
                __syncthreads();
                ddpg_backward<true>(G.params, L.critic[j], L.Kc, 1, Xs, H1, H2, Gb, Tb, dO, g[j], tid);
            }
        }
    }
    float* S = G.slab + (size_t)blockIdx.x * L.SW;
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (j < L.NC) ddpg_store(S, L.critic[j], L.Kc, 1, g[j], tid);
    __syncthreads();
    if (tid < FWG_PPO_ROWS) { rowf[tid * 8 + 0] = st[0]; rowf[tid * 8 + 1] = st[1]; rowf[tid * 8 + 2] = st[2]; }
    __syncthreads();
    if (tid < 3) {   // the 64 lanes' sums in lane order
        float s = 0.f;
        for (int r = 0; r < FWG_PPO_ROWS; ++r) s += rowf[r * 8 + tid];
        S[L.P + (tid == 0 ? 0 : tid + 1)] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ddpg_actor_grad: L_a = -mean Q_0(o, g, pi(o, g)).  The critic's weight gradients are neither formed nor written
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ddpg_actor_grad(const DdpgGradArgs G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LS = FWG_PPO_LS;
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const DdpgLayout& L = G.L;
    float* Xs = lds;                         // [64][LS] [o | g | pi]
    float* H1a = Xs + FWG_PPO_ROWS * LS;     // [64][LS] the actor's hidden layers
    float* H2a = H1a + FWG_PPO_ROWS * LS;
    float* H1c = H2a + FWG_PPO_ROWS * LS;    // [64][LS] the critic's; H1c is the actor's dL / d(pre-activation 1) afterwards
    float* H2c = H1c + FWG_PPO_ROWS * LS;    //           H2c is the critic's dQ / d(pre-activation 1) afterwards
    float* Gb = H2c + FWG_PPO_ROWS * LS;     // [64][LS] dL / d(pre-activation 2) of the network in flight
    float* dO = Gb + FWG_PPO_ROWS * LS;      // [64][4]
    float* rowf = dO + 4 * FWG_PPO_ROWS;     // [64][8] pi[4]; at the end the reduction space
    const float inv_n = 1.f / (float)G.n;
    const long t0 = (long)blockIdx.x * G.ntiles / gridDim.x, t1 = (long)(blockIdx.x + 1) * G.ntiles / gridDim.x;
    DdpgAcc g, none;
    ddpg_acc_zero(g);
    float sq = 0.f;
    for (long t = t0; t < t1; ++t) {
        const long r0 = t * FWG_PPO_ROWS;
        const int nrows = (int)(G.n - r0 < FWG_PPO_ROWS ? G.n - r0 : FWG_PPO_ROWS);
        const bool ok = tid < nrows;
        ddpg_gather(Xs, L, G.B.obs, G.B.goal, nullptr, r0, nrows, tid);
        __syncthreads();
        ddpg_forward<true>(G.params, L.actor, L.Ka, L.A, Xs, H1a, H2a, dO, tid);
        if (tid < FWG_PPO_ROWS)
            for (int a = 0; a < L.A; ++a) { const float p = dO[tid * 4 + a]; rowf[tid * 8 + a] = p; Xs[tid * LS + L.Ka + a] = p; }
        __syncthreads();
        ddpg_forward<false>(G.params, L.critic[0], L.Kc, 1, Xs, H1c, H2c, dO, tid);
        if (tid < FWG_PPO_ROWS) {
            if (ok) sq += dO[tid * 4];
            dO[tid * 4] = ok ? -inv_n : 0.f;   // dL_a / dQ
        }
        __syncthreads();
        ddpg_backward<false>(G.params, L.critic[0], L.Kc, 1, Xs, H1c, H2c, Gb, H2c, dO, none, tid);
        if (wv < L.A) {   // dL / da = G1 W1[:, Ka + a] (the action columns only), then through tanh: column wv of row l
            const float* W1 = G.params + L.critic[0].w1 + L.Ka + wv;
            float s = 0.f;
#pragma unroll 8
            for (int k = 0; k < 64; ++k) s += H2c[l * LS + k] * W1[k * L.Kc];
            const float p = rowf[l * 8 + wv];
            dO[l * 4 + wv] = s * (1.f - p * p);
        }
        __syncthreads();
        ddpg_backward<true>(G.params, L.actor, L.Ka, L.A, Xs, H1a, H2a, Gb, H1c, dO, g, tid);
    }
    float* S = G.slab + (size_t)blockIdx.x * L.SW;
    ddpg_store(S, L.actor, L.Ka, L.A, g, tid);
    __syncthreads();
    if (tid < FWG_PPO_ROWS) rowf[tid * 8] = sq;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int r = 0; r < FWG_PPO_ROWS; ++r) s += rowf[r * 8];
        S[L.P + 1] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ddpg_reduce: one segment of grad (seg 0: the actor's [0, PA) and loss sum 1; seg 1: the critics' [PA, P) and loss sums 0, 2, 3)
// = the sum over the slabs in index order.  The other segment's words are not touched
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ddpg_reduce(const float* __restrict__ slab, int nslab, const DdpgLayout L, int seg,
                                                                 float* __restrict__ grad) {
    const int j = blockIdx.x * FWG_PPO_THREADS + threadIdx.x;
    const int lo = seg ? L.PA : 0, n = seg ? L.P - L.PA : L.PA;
    int idx;
    if (j < n) idx = lo + j;
    else if (j < n + FWG_DDPG_NSTAT) {
        const int s = j - n;
        if ((s == 1) != (seg == 0)) return;
        idx = L.P + s;
    } else return;
    float s = 0.f;
    for (int b = 0; b < nslab; ++b) s += slab[(size_t)b * L.SW + idx];
    grad[idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ddpg_apply (one workgroup): Adam on one segment, k_ppo_apply's form -- m = m + (1 - b1) (g - m), v = b2 v + (1 - b2) g^2,
// p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) with t = step[seg] + 1; max_norm > 0: clip_grad_norm_ over the segment
// first.  acc[4] (critic_loss, actor_loss, q_mean, target_mean) += the segment's statistics of this batch of n rows
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWG_PPO_APPLY_THREADS) void k_ddpg_apply(const float* __restrict__ grad, long n, const DdpgLayout L, int seg,
                                                                      const DdpgHparams h, float* __restrict__ params, float* __restrict__ m1,
                                                                      float* __restrict__ m2, int* __restrict__ step, float* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lo = seg ? L.PA : 0, hi = seg ? L.P : L.PA;
    const float max_norm = (float)(seg ? h.max_norm_critic : h.max_norm_actor);
    float coef = 1.f;
    if (max_norm > 0.f) {
        float ss = 0.f;
        for (int j = lo + tid; j < hi; j += FWG_PPO_APPLY_THREADS) ss += grad[j] * grad[j];
        lds[tid] = ss;
        __syncthreads();
        for (int w = FWG_PPO_APPLY_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) lds[tid] += lds[tid + w];
            __syncthreads();
        }
        coef = fminf(max_norm / (sqrtf(lds[0]) + 1e-6f), 1.f);
    }
    const int t = step[seg] + 1;
    const double lr = seg ? h.lr_critic : h.lr_actor;
    const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float b2 = (float)h.beta2, w1 = (float)(1.0 - h.beta1), w2 = (float)(1.0 - h.beta2), eps = (float)h.eps;
    for (int j = lo + tid; j < hi; j += FWG_PPO_APPLY_THREADS) {
        const float gj = grad[j] * coef;
        float m = m1[j], v = m2[j];
        m = m + w1 * (gj - m);
        v = v * b2 + w2 * (gj * gj);
        m1[j] = m; m2[j] = v;
        params[j] -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
    }
    __syncthreads();
    if (tid == 0) {
        const float inv = 1.f / (float)n;
        step[seg] = t;
        if (seg) {
            acc[0] += grad[L.P] * inv;
            acc[2] += grad[L.P + 2] * inv;
            acc[3] += grad[L.P + 3] * inv;
        } else acc[1] -= grad[L.P + 1] * inv;
    }
}

// k_ddpg_polyak: target <- lerp(target, params, tau), torch's lerp_ (weight < 0.5: start + w (end - start), else end - (end - start) (1 - w))
__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ddpg_polyak(const float* __restrict__ params, float* __restrict__ target, int P, float tau) {
    const int j = blockIdx.x * FWG_PPO_THREADS + threadIdx.x;
    if (j >= P) return;
    const float p = params[j], t = target[j], d = p - t;
    target[j] = tau < 0.5f ? t + tau * d : p - d * (1.f - tau);
}
