// fwgym_learner.h -- the PPO update on the device (include/fwgym.h "PPO update"): stable-baselines PPO2's minibatch step
// (ppo2.py setup_model: per-minibatch advantage normalisation, clipped surrogate, value loss clipped around the old value
// with the same range, Gaussian entropy of the state-independent log-std), clip_grad_norm_ and torch.optim.Adam(eps=1e-5)
// on the 64-64 MlpPolicy of the rollout head.  Five kernels, one stream, no grid-wide barrier:
//   k_ppo_moments : once per epoch, mean and biased std (+1e-8) of the advantages of every minibatch of a permutation
//   k_ppo_grad    : the hot path.  A workgroup walks 64-row tiles of the minibatch (rows gathered by index straight from the
//                   step-major rollout buffers), runs pi and vf forward, the loss terms, and the backward pass, and writes
//                   ONE fp32 partial gradient slab (+ four loss sums) per workgroup
//   k_ppo_reduce  : sums the slabs in a fixed order (no float atomics: the update is bitwise deterministic run to run)
//   k_ppo_apply   : global gradient norm, clip, Adam on the fp32 master parameters, statistics
//   k_actor_pack  : the head's operand fragments / biases / log-std (fwg_actor_set_weights' packing) from the flat parameters
// Parameters, gradients and Adam moments share one flat fp32 layout, MlpPolicy.parameters() order:
//   log_std | pi.0.weight pi.0.bias pi.2.weight pi.2.bias pi.4.weight pi.4.bias | vf.0.weight ... vf.4.bias
// and for the CNN head's CnnMlpPolicy (fwg_learner_create_cnn, k_ppo_grad<true>), CnnMlpPolicy.parameters() order:
//   log_std | conv.weight [5][3] conv.bias [3] | pi.1.weight [64][36] pi.1.bias ... pi.5.bias | vf.1.weight ... vf.5.bias
// The conv (one module shared by pi and vf) runs on the VALU: C = tanh(conv(X)) in a sixth LDS tile is the networks' input, the
// two networks' dL / dC add up in one accumulator carried over the per-network loop, and the 18 conv gradients are per-lane
// partial sums over the workgroup's tiles, reduced in a fixed order at the end.
// The GEMMs run on v_mfma_f32_32x32x16_bf16 with every fp32 operand split x = hi + lo (three products, fwgym_actor.h).  A tile's
// activations sit in LDS row-major (stride FWG_PPO_LS, odd: row-strided lane reads hit distinct banks); each of the four waves
// owns one 32x32 quarter of every 64x64 product, so the weight-gradient GEMMs (contraction over the tile's rows) accumulate in
// the same registers across all the tiles of a workgroup.
#pragma once
#include "fwgym_actor.h"

#define FWG_PPO_ROWS 64            // rows per tile
#define FWG_PPO_THREADS 256        // four waves
#define FWG_PPO_MAX_BLOCKS 256     // partial-gradient slabs (one workgroup per CU at most)
#define FWG_PPO_LS 65              // LDS row stride of the [64][64] activation tiles, floats
#define FWG_PPO_NSTAT 4            // per-slab loss sums: pg, vf, approx-kl, clipped count (the entropy comes from log_std)
#define FWG_PPO_APPLY_THREADS 256

// (double: the values torch.optim.Adam / clip_grad_norm_ compute their scalars from -- 1 - beta2 of a float beta2 is off by 1e-5)
struct PpoHparams { double lr, cliprange, ent_coef, vf_coef, max_grad_norm, beta1, beta2, eps; };
// offsets into the flat parameter vector; [net] 0 = pi, 1 = vf.  P parameters, SW floats per slab (P + the loss sums, padded)
// K1: layer 0's fan-in (D; the CNN's 36 conv outputs).  cnn: 1 = the conv's weight [5][3] at cw and bias [3] at cb
struct PpoLayout { int D, A, P, SW; int ls, w1[2], b1[2], w2[2], b2[2], w3[2], b3[2]; int K1, cnn, cw, cb; };
struct PpoBatch { const float *obs, *act, *val, *logp, *adv, *ret; };

__host__ __device__ inline PpoLayout ppo_layout(int D, int A, bool cnn = false) {
    PpoLayout L;
    L.D = D; L.A = A;
    L.K1 = cnn ? FWG_CNN_K : D; L.cnn = cnn ? 1 : 0; L.cw = L.cb = 0;
    int o = 0;
    L.ls = o; o += A;
    if (cnn) {
        L.cw = o; o += FWG_CNN_ROWS * FWG_CNN_FILTERS;
        L.cb = o; o += FWG_CNN_FILTERS;
    }
    for (int net = 0; net < 2; ++net) {
        const int nout = net ? 1 : A;
        L.w1[net] = o; o += 64 * L.K1;
        L.b1[net] = o; o += 64;
        L.w2[net] = o; o += 64 * 64;
        L.b2[net] = o; o += 64;
        L.w3[net] = o; o += nout * 64;
        L.b3[net] = o; o += nout;
    }
    L.P = o;
    L.SW = (o + FWG_PPO_NSTAT + 3) & ~3;
    return L;
}

// tanh on the VALU: 1 - 2 / (2^(2 log2(e) z) + 1), absolute error ~1e-7
__device__ __forceinline__ float ppo_tanh(float z) { return tanh_prescaled(FWG_ACT_PRESCALE * z); }

// acc += sum_k A(m, k) B(k, n) for the calling wave's 32 x 32 tile (m0, n0), A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn],
// k over [0, K) in 16-wide blocks; entries with m >= ml, k >= kl or n >= nl read as 0 (and are not addressed).  Lane l
// supplies A row / B column l & 31 and k-slots 8 (l >> 5) + t; it receives rows (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
// ROLLED (the CNN instance of k_ppo_grad): two k-blocks unrolled instead of all -- with every block's operand loads hoisted the
// CNN instance needs more than the 512 registers of a lane; the default leaves the MLP instance's code as it was
template <bool ROLLED = false>
__device__ __forceinline__ void ppo_mma_tile(f32x16& acc, const float* A, int sam, int sak, int m0, int ml, const float* B, int sbk,
                                             int sbn, int n0, int nl, int K, int kl, int l) {
    const int i = l & 31, half = l >> 5;
    const bool mok = m0 + i < ml, nok = n0 + i < nl;
#pragma unroll (ROLLED ? 2 : 8)
    for (int k0 = 0; k0 < K; k0 += 16) {
        float a[8], b[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = k0 + 8 * half + t;
            a[t] = (mok && k < kl) ? A[(m0 + i) * sam + k * sak] : 0.f;
            b[t] = (nok && k < kl) ? B[k * sbk + (n0 + i) * sbn] : 0.f;
        }
        frag_t ah, al, bh, bl;
        split8(a, ah, al);
        split8(b, bh, bl);
        acc = mma3<3>(ah, al, bh, bl, acc);
    }
}
__device__ __forceinline__ int ppo_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---------------------------------------------------------------------------------------------------------------------
// k_ppo_moments: block k = minibatch k of the permutation; two passes in double, fixed-order tree (deterministic).
// mom[2k] = mean, mom[2k + 1] = std (biased) + 1e-8 of adv[perm[k mb ... (k + 1) mb)]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ppo_moments(const float* __restrict__ adv, const long long* __restrict__ perm,
                                                                 long mb, float* __restrict__ mom) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    double* red = reinterpret_cast<double*>(lds);
    const int tid = threadIdx.x;
    const long long* idx = perm + (long)blockIdx.x * mb;
    double s = 0.0;
    for (long i = tid; i < mb; i += FWG_PPO_THREADS) s += (double)adv[idx[i]];
    red[tid] = s;
    __syncthreads();
    for (int w = FWG_PPO_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double mean = red[0] / (double)mb;
    __syncthreads();
    double q = 0.0;
    for (long i = tid; i < mb; i += FWG_PPO_THREADS) {
        const double d = (double)adv[idx[i]] - mean;
        q += d * d;
    }
    red[tid] = q;
    __syncthreads();
    for (int w = FWG_PPO_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        mom[2 * blockIdx.x] = (float)mean;
        mom[2 * blockIdx.x + 1] = (float)sqrt(red[0] / (double)mb) + 1e-8f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ppo_grad
// ---------------------------------------------------------------------------------------------------------------------
struct PpoGradArgs {
    PpoBatch B;
    const long long* idx;       // [mb] rows of this minibatch (into the flattened [n_steps x n_envs] buffers)
    long mb;
    long ntiles;                // ceil(mb / 64), spread evenly over gridDim.x workgroups
    const float* mom;           // [2] mean, std + 1e-8 of this minibatch's advantages
    const float* params;
    const PpoHparams* hp;
    float* slab;                // [gridDim.x][SW]
    PpoLayout L;
};
// (CNN: one more tile, the conv outputs)
__host__ __device__ inline int ppo_grad_lds_floats(bool cnn = false) {
    return (cnn ? 6 : 5) * FWG_PPO_ROWS * FWG_PPO_LS + 4 * FWG_PPO_ROWS + 8 * FWG_PPO_ROWS + 8 * FWG_PPO_ROWS;
}
#define FWG_PPO_CNN_SUMS (FWG_CNN_ROWS * FWG_CNN_FILTERS + FWG_CNN_FILTERS)   // conv gradients: dW [5][3], then db [3]
#define FWG_PPO_CNN_PARTS 8                                                   // ... each summed by 8 lanes, 8 rows of a tile each

// CNN = true: the CnnMlpPolicy's instance.  Its loops are unrolled by 8 / 2 (`CNN ? 8 : 64`: 64 = all of it, the MLP instance's
// code is what it was before the template): 248-256 VGPRs, no scratch, no spills (gym_fixed_wing/kernel_resources.json)
template <bool CNN>
__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ppo_grad(const PpoGradArgs G) {
    // (the backward pass below differentiates tanh, and both passes index the conv outputs feature-major)
    static_assert(!CNN || (FWG_CNN_ACTIVATION == FWG_CNN_ACT_TANH && FWG_CNN_FEATURE_MAJOR == 1), "k_ppo_grad<true>: tanh after the conv, k = j * FILTERS + c");
    static_assert(FWG_PPO_CNN_SUMS * FWG_PPO_CNN_PARTS <= FWG_PPO_THREADS && FWG_PPO_CNN_SUMS * FWG_PPO_CNN_PARTS <= 8 * FWG_PPO_ROWS &&
                  FWG_CNN_ROWS * FWG_CNN_COLS <= 64 && FWG_CNN_K <= 64, "conv gradient lanes / reduction space / tile width");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LS = FWG_PPO_LS;
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, half = l >> 5;
    const PpoLayout& L = G.L;
    const int D = L.D, A = L.A, nk1 = (D + 15) / 16;
    float* Xs = lds;                        // [64][LS] observations of the tile (0 beyond D and beyond the last row)
    float* H1 = Xs + FWG_PPO_ROWS * LS;     // [64][LS] first hidden layer
    float* H2 = H1 + FWG_PPO_ROWS * LS;     // [64][LS] second hidden layer
    float* Gb = H2 + FWG_PPO_ROWS * LS;     // [64][LS] dL / d(pre-activation 2)
    float* Tb = Gb + FWG_PPO_ROWS * LS;     // [64][LS] dL / d(pre-activation 1)
    float* dO = Tb + FWG_PPO_ROWS * LS;     // [64][4] network outputs, then dL / d(output)
    float* rowf = dO + 4 * FWG_PPO_ROWS;    // [64][8] action[4], old value, old log-prob, normalised advantage, return
    float* red = rowf + 8 * FWG_PPO_ROWS;   // [64][8] end-of-block reduction of the per-row sums
    float* Cs = red + 8 * FWG_PPO_ROWS;     // (CNN) [64][LS] conv outputs of the tile, k = feature * FILTERS + filter
    const PpoHparams hp = *G.hp;
    const float adv_mean = G.mom[0], adv_std = G.mom[1];
    const float inv_mb = 1.f / (float)G.mb, clip = (float)hp.cliprange, vf_coef = (float)hp.vf_coef;
    const float* P = G.params;
    const long t0 = (long)blockIdx.x * G.ntiles / gridDim.x, t1 = (long)(blockIdx.x + 1) * G.ntiles / gridDim.x;
    const int tm0 = 32 * (wv & 1), tn0 = 32 * (wv >> 1);   // this wave's quarter of every 64 x 64 product
    const int vo = tid >> 6, vk = tid & 63;                // (output unit, hidden unit) of the output layer's VALU work
    f32x16 gw1[2], gw2[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { gw1[0][r] = 0.f; gw1[1][r] = 0.f; gw2[0][r] = 0.f; gw2[1][r] = 0.f; }
    float gw3[2] = {0.f, 0.f}, gb3[2] = {0.f, 0.f}, gb2[2] = {0.f, 0.f}, gb1[2] = {0.f, 0.f};
    float gls[FWG_ACT_MAX_ACT] = {0.f, 0.f, 0.f, 0.f}, st[FWG_PPO_NSTAT] = {0.f, 0.f, 0.f, 0.f};
    // (CNN) conv gradient `cs` (r * FILTERS + c: dW[r][c]; ROWS * FILTERS + c: db[c]) over the tile rows 8 cp .. 8 cp + 7
    const int cs = tid / FWG_PPO_CNN_PARTS, cp = tid % FWG_PPO_CNN_PARTS;
    float gcv = 0.f;
    for (long t = t0; t < t1; ++t) {
        const long r0 = t * FWG_PPO_ROWS;
        const int nrows = (int)(G.mb - r0 < FWG_PPO_ROWS ? G.mb - r0 : FWG_PPO_ROWS);
        {   // gather: four threads per row, 16 features each; the first of them takes the row's scalars
            const int r = tid >> 2, q = tid & 3;
            const bool ok = r < nrows;
            const long long row = ok ? G.idx[r0 + r] : 0;
            for (int f = 16 * q; f < 16 * q + 16; ++f) Xs[r * LS + f] = (ok && f < D) ? G.B.obs[row * D + f] : 0.f;
            if (q == 0) {
#pragma unroll
                for (int a = 0; a < FWG_ACT_MAX_ACT; ++a) rowf[r * 8 + a] = (ok && a < A) ? G.B.act[row * A + a] : 0.f;
                rowf[r * 8 + 4] = ok ? G.B.val[row] : 0.f;
                rowf[r * 8 + 5] = ok ? G.B.logp[row] : 0.f;
                rowf[r * 8 + 6] = ok ? (G.B.adv[row] - adv_mean) / adv_std : 0.f;
                rowf[r * 8 + 7] = ok ? G.B.ret[row] : 0.f;
            }
        }
        __syncthreads();
        f32x16 dc = {0.f};   // (CNN) dL / dC of this wave's quarter, both networks
        if constexpr (CNN) {   // C = tanh(conv(X)): 64 rows x 36 outputs, nine per thread (rows past the minibatch: X = 0)
            const float *cw = P + L.cw, *cb = P + L.cb;
#pragma unroll 1
            for (int e = tid; e < FWG_PPO_ROWS * FWG_CNN_K; e += FWG_PPO_THREADS) {
                const int r = e / FWG_CNN_K, k = e % FWG_CNN_K, j = cnn_feature(k), c = cnn_filter(k);
                float z = cb[c];
#pragma unroll
                for (int q = 0; q < FWG_CNN_ROWS; ++q) z = fmaf(cw[q * FWG_CNN_FILTERS + c], Xs[r * LS + q * FWG_CNN_COLS + j], z);
                Cs[r * LS + k] = ppo_tanh(z);
            }
            __syncthreads();
        }
#pragma unroll
        for (int net = 0; net < 2; ++net) {   // (unrolled: the per-network accumulators stay in registers)
            const int nout = net ? 1 : A;
            const float *W1 = P + L.w1[net], *b1 = P + L.b1[net], *W2 = P + L.w2[net], *b2 = P + L.b2[net];
            const float *W3 = P + L.w3[net], *b3 = P + L.b3[net];
            {   // layer 1: H1 = tanh(X W1^T + b1)
                f32x16 acc = {0.f};
                if constexpr (CNN) ppo_mma_tile<CNN>(acc, Cs, LS, 1, tm0, 64, W1, 1, FWG_CNN_K, tn0, 64, 16 * FWG_CNN_NK1, FWG_CNN_K, l);
                else
                ppo_mma_tile<CNN>(acc, Xs, LS, 1, tm0, 64, W1, 1, D, tn0, 64, 16 * nk1, D, l);
                const int n = tn0 + (l & 31);
                const float bn = b1[n];
#pragma unroll
                for (int r = 0; r < 16; ++r) H1[(tm0 + ppo_acc_row(r, half)) * LS + n] = ppo_tanh(acc[r] + bn);
            }
            __syncthreads();
            {   // layer 2: H2 = tanh(H1 W2^T + b2)
                f32x16 acc = {0.f};
                ppo_mma_tile<CNN>(acc, H1, LS, 1, tm0, 64, W2, 1, 64, tn0, 64, 64, 64, l);
                const int n = tn0 + (l & 31);
                const float bn = b2[n];
#pragma unroll
                for (int r = 0; r < 16; ++r) H2[(tm0 + ppo_acc_row(r, half)) * LS + n] = ppo_tanh(acc[r] + bn);
            }
            __syncthreads();
            if (vo < nout) {   // output layer (act_dim <= 4 / 1 columns: VALU), row vk
                float o = b3[vo];
#pragma unroll (CNN ? 8 : 64)
                for (int k = 0; k < 64; ++k) o += H2[vk * LS + k] * W3[vo * 64 + k];
                dO[vk * 4 + vo] = o;
            }
            __syncthreads();
            if (tid < FWG_PPO_ROWS) {   // loss terms and dL / d(output) of row tid; rows past the minibatch contribute nothing
                const int r = tid;
                const bool ok = r < nrows;
                const float* rf = rowf + r * 8;
                if (net == 0) {
                    // neglogp = 0.5 sum ((a - mu) / sigma)^2 + 0.5 log(2 pi) A + sum log_std; ratio = exp(old logp - neglogp)
                    float nl = 0.9189385332046727f * (float)A, z[FWG_ACT_MAX_ACT], is[FWG_ACT_MAX_ACT];
#pragma unroll
                    for (int a = 0; a < FWG_ACT_MAX_ACT; ++a) {
                        z[a] = 0.f; is[a] = 0.f;
                        if (a < A) {
                            const float s = P[L.ls + a];
                            is[a] = expf(-s);
                            z[a] = (rf[a] - dO[r * 4 + a]) * is[a];
                            nl += 0.5f * z[a] * z[a] + s;
                        }
                    }
                    const float ratio = expf(-rf[5] - nl), adv = rf[6];
                    const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
                    const float p1 = -adv * ratio, p2 = -adv * rc;
                    // d max(p1, p2) / d ratio (torch: a tie splits the gradient; clamp passes it inside [1 - c, 1 + c] inclusive)
                    const float g1 = -adv, g2 = (ratio >= 1.f - clip && ratio <= 1.f + clip) ? -adv : 0.f;
                    const float dr = p1 > p2 ? g1 : (p1 < p2 ? g2 : 0.5f * (g1 + g2));
                    const float gn = ok ? -ratio * dr * inv_mb : 0.f;   // dL / d neglogp
#pragma unroll
                    for (int a = 0; a < FWG_ACT_MAX_ACT; ++a) {
                        dO[r * 4 + a] = a < A ? -gn * z[a] * is[a] : 0.f;   // d neglogp / d mu = -(a - mu) / sigma^2
                        gls[a] += a < A ? gn * (1.f - z[a] * z[a]) : 0.f;   // d neglogp / d log_std = 1 - z^2
                    }
                    if (ok) {
                        const float kl = nl + rf[5];
                        st[0] += fmaxf(p1, p2);
                        st[2] += 0.5f * kl * kl;
                        st[3] += fabsf(ratio - 1.f) > clip ? 1.f : 0.f;
                    }
                } else {
                    const float v = dO[r * 4], ov = rf[4], R = rf[7], d = v - ov;
                    const float vc = ov + fminf(fmaxf(d, -clip), clip);
                    const float l1 = (v - R) * (v - R), l2 = (vc - R) * (vc - R);
                    const float g1 = 2.f * (v - R), g2 = (d >= -clip && d <= clip) ? 2.f * (vc - R) : 0.f;
                    const float dv = l1 > l2 ? g1 : (l1 < l2 ? g2 : 0.5f * (g1 + g2));
                    dO[r * 4] = ok ? vf_coef * 0.5f * dv * inv_mb : 0.f;
                    if (ok) st[1] += 0.5f * fmaxf(l1, l2);
                }
            }
            __syncthreads();
            // ---- backward: output layer (VALU)
            if (vo < nout) {
                float s = 0.f, sb = 0.f;
#pragma unroll (CNN ? 8 : 64)
                for (int r = 0; r < FWG_PPO_ROWS; ++r) { s += dO[r * 4 + vo] * H2[r * LS + vk]; sb += dO[r * 4 + vo]; }
                gw3[net] += s;
                if (vk == 0) gb3[net] += sb;
            }
            // G2 = (dO W3) * (1 - H2^2)
#pragma unroll (CNN ? 8 : 64)
            for (int j = 0; j < FWG_PPO_ROWS * 64 / FWG_PPO_THREADS; ++j) {
                const int e = tid + FWG_PPO_THREADS * j, r = e >> 6, k = e & 63;
                float s = 0.f;
                for (int o = 0; o < nout; ++o) s += dO[r * 4 + o] * W3[o * 64 + k];
                const float h = H2[r * LS + k];
                Gb[r * LS + k] = s * (1.f - h * h);
            }
            __syncthreads();
            {   // G1 = (G2 W2) * (1 - H1^2);  dW2 += G2^T H1 (contraction over the tile's rows);  db2
                f32x16 acc = {0.f};
                ppo_mma_tile<CNN>(acc, Gb, LS, 1, tm0, 64, W2, 64, 1, tn0, 64, 64, 64, l);
                const int n = tn0 + (l & 31);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tm0 + ppo_acc_row(r, half);
                    const float h = H1[m * LS + n];
                    Tb[m * LS + n] = acc[r] * (1.f - h * h);
                }
                ppo_mma_tile<CNN>(gw2[net], Gb, 1, LS, tm0, 64, H1, LS, 1, tn0, 64, 64, 64, l);
                if (tid < 64) {
                    float s = 0.f;
#pragma unroll (CNN ? 8 : 64)
                    for (int r = 0; r < FWG_PPO_ROWS; ++r) s += Gb[r * LS + tid];
                    gb2[net] += s;
                }
            }
            __syncthreads();
            // dW1 += G1^T X;  db1  (CNN: G1^T C, and dC += G1 W1 -- the conv is shared, the two networks' terms add)
            if constexpr (CNN) {
                ppo_mma_tile<CNN>(gw1[net], Tb, 1, LS, tm0, 64, Cs, LS, 1, tn0, FWG_CNN_K, 64, 64, l);
                ppo_mma_tile<CNN>(dc, Tb, LS, 1, tm0, 64, W1, FWG_CNN_K, 1, tn0, FWG_CNN_K, 64, 64, l);
            } else
            if (tn0 < D) ppo_mma_tile<CNN>(gw1[net], Tb, 1, LS, tm0, 64, Xs, LS, 1, tn0, D, 64, 64, l);
            if (tid < 64) {
                float s = 0.f;
#pragma unroll (CNN ? 8 : 64)
                for (int r = 0; r < FWG_PPO_ROWS; ++r) s += Tb[r * LS + tid];
                gb1[net] += s;
            }
            __syncthreads();
        }
        if constexpr (CNN) {   // dZ = dC * (1 - C^2) into Gb (free by now), then the conv's gradients: contraction over rows and features
            const int n = tn0 + (l & 31);
            if (n < FWG_CNN_K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = tm0 + ppo_acc_row(r, half);
                    const float c = Cs[m * LS + n];
                    Gb[m * LS + n] = dc[r] * (1.f - c * c);
                }
            }
            __syncthreads();
            if (cs < FWG_PPO_CNN_SUMS) {
                const bool isw = cs < FWG_CNN_ROWS * FWG_CNN_FILTERS;
                const int q = isw ? cs / FWG_CNN_FILTERS : 0, c = isw ? cs % FWG_CNN_FILTERS : cs - FWG_CNN_ROWS * FWG_CNN_FILTERS;
                float s = 0.f;
#pragma unroll 1
                for (int r = FWG_PPO_ROWS / FWG_PPO_CNN_PARTS * cp; r < FWG_PPO_ROWS / FWG_PPO_CNN_PARTS * (cp + 1); ++r)
                    for (int j = 0; j < FWG_CNN_COLS; ++j)
                        s += Gb[r * LS + j * FWG_CNN_FILTERS + c] * (isw ? Xs[r * LS + q * FWG_CNN_COLS + j] : 1.f);
                gcv += s;
            }
            __syncthreads();   // (the next tile's gather writes Xs)
        }
    }
    // ---- the workgroup's slab: every entry written by exactly one lane
    float* S = G.slab + (size_t)blockIdx.x * L.SW;
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        const int nout = net ? 1 : A;
        const int n = tn0 + (l & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = tm0 + ppo_acc_row(r, half);
            if constexpr (CNN) { if (n < FWG_CNN_K) S[L.w1[net] + m * FWG_CNN_K + n] = gw1[net][r]; } else
            if (n < D) S[L.w1[net] + m * D + n] = gw1[net][r];
            S[L.w2[net] + m * 64 + n] = gw2[net][r];
        }
        if (vo < nout) {
            S[L.w3[net] + vo * 64 + vk] = gw3[net];
            if (vk == 0) S[L.b3[net] + vo] = gb3[net];
        }
        if (tid < 64) { S[L.b1[net] + tid] = gb1[net]; S[L.b2[net] + tid] = gb2[net]; }
    }
    if (tid < FWG_PPO_ROWS) {
#pragma unroll
        for (int a = 0; a < 4; ++a) { red[tid * 8 + a] = gls[a]; red[tid * 8 + 4 + a] = st[a]; }
    }
    __syncthreads();
    if (tid < 8) {
        float s = 0.f;
        for (int r = 0; r < FWG_PPO_ROWS; ++r) s += red[r * 8 + tid];
        if (tid < A) S[L.ls + tid] = s;
        else if (tid >= 4) S[L.P + tid - 4] = s;
    }
    if constexpr (CNN) {   // the conv's 18 gradients: the 8 lanes' partial sums in lane order (conv.weight and conv.bias are adjacent)
        __syncthreads();
        if (cs < FWG_PPO_CNN_SUMS) red[tid] = gcv;
        __syncthreads();
        if (tid < FWG_PPO_CNN_SUMS) {
            float s = 0.f;
            for (int p = 0; p < FWG_PPO_CNN_PARTS; ++p) s += red[tid * FWG_PPO_CNN_PARTS + p];
            S[L.cw + tid] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ppo_reduce: grad[j] = sum over the slabs in index order (+ the entropy term -ent_coef on log_std), j < P + NSTAT
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWG_PPO_THREADS) void k_ppo_reduce(const float* __restrict__ slab, int nslab, const PpoLayout L,
                                                                const PpoHparams* __restrict__ hp, float* __restrict__ grad) {
    const int j = blockIdx.x * FWG_PPO_THREADS + threadIdx.x;
    if (j >= L.P + FWG_PPO_NSTAT) return;
    float s = 0.f;
    for (int b = 0; b < nslab; ++b) s += slab[(size_t)b * L.SW + j];
    if (j >= L.ls && j < L.ls + L.A) s -= (float)hp->ent_coef;   // d(-ent_coef * entropy) / d log_std
    grad[j] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ppo_apply (one workgroup): clip_grad_norm_(max_norm): coef = min(max_norm / (||g|| + 1e-6), 1); Adam, torch's form:
// m = m + (1 - b1) (g - m), v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), t on the
// device.  acc[5] += the minibatch's pg_loss, vf_loss, entropy (of the log_std BEFORE the step), approx_kl, clip_frac
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWG_PPO_APPLY_THREADS) void k_ppo_apply(const float* __restrict__ grad, long mb, const PpoLayout L,
                                                                     const PpoHparams* __restrict__ hp, float* __restrict__ params,
                                                                     float* __restrict__ m1, float* __restrict__ m2, int* __restrict__ step,
                                                                     float* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    float ent = 0.f;
    if (tid == 0)
        for (int a = 0; a < L.A; ++a) ent += params[L.ls + a] + 1.4189385332046727f;   // log_std + 0.5 log(2 pi e)
    float ss = 0.f;
    for (int j = tid; j < L.P; j += FWG_PPO_APPLY_THREADS) ss += grad[j] * grad[j];
    lds[tid] = ss;
    __syncthreads();
    for (int w = FWG_PPO_APPLY_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) lds[tid] += lds[tid + w];
        __syncthreads();
    }
    const PpoHparams h = *hp;
    const float norm = sqrtf(lds[0]);
    const float coef = fminf((float)h.max_grad_norm / (norm + 1e-6f), 1.f);
    const int t = *step + 1;
    const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
    const float step_size = (float)(h.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float b2 = (float)h.beta2, w1 = (float)(1.0 - h.beta1), w2 = (float)(1.0 - h.beta2), eps = (float)h.eps;
    for (int j = tid; j < L.P; j += FWG_PPO_APPLY_THREADS) {
        const float g = grad[j] * coef;
        float m = m1[j], v = m2[j];
        m = m + w1 * (g - m);
        v = v * b2 + w2 * (g * g);
        m1[j] = m; m2[j] = v;
        params[j] -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
    }
    __syncthreads();
    if (tid == 0) {
        const float inv = 1.f / (float)mb;
        *step = t;
        acc[0] += grad[L.P] * inv;
        acc[1] += grad[L.P + 1] * inv;
        acc[2] += ent;
        acc[3] += grad[L.P + 2] * inv;
        acc[4] += grad[L.P + 3] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_actor_pack: fwg_actor_set_weights' packing (actor_pack_layer / actor_pack_bias) on the device, from the flat parameters.
// Thread = (net, fragment, lane) of frags [net][part hi/lo][frag][64]; the last 2 x FWG_ACT_BIAS_FLOATS + 4 threads write the
// biases and the log-std; for a CNN layout FWG_CNN_PARAMS more write the conv behind the biases (fwg_actor_set_conv's layout)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_actor_pack(const float* __restrict__ params, const PpoLayout L, int nk1, frag_t* __restrict__ frags,
                                                    float* __restrict__ bias, float* __restrict__ log_std) {
    const int nfw = actor_frags(nk1);
    const int nfrag_thr = 2 * nfw * 64;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < nfrag_thr) {
        const int net = g / (nfw * 64), f = (g / 64) % nfw, l = g & 63, half = l >> 5;
        const int nout = net ? 1 : L.A;
        const float* W;
        int out, in, it, kk;
        bool chained;
        float scale;
        if (f < 2 * nk1) { W = params + L.w1[net]; out = 64; in = L.K1; it = f / nk1; kk = f % nk1; chained = false; scale = FWG_ACT_PRESCALE; }
        else if (f < 2 * nk1 + 8) { W = params + L.w2[net]; out = 64; in = 64; it = (f - 2 * nk1) / 4; kk = (f - 2 * nk1) % 4; chained = true; scale = FWG_ACT_PRESCALE; }
        else { W = params + L.w3[net]; out = nout; in = 64; it = 0; kk = f - 2 * nk1 - 8; chained = true; scale = 1.f; }
        const int i = 32 * it + (l & 31);
        unsigned wh[4] = {0u, 0u, 0u, 0u}, wl[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = chained ? k_chained(kk, half, t) : k_input(kk, half, t);
            const float v = (i < out && k < in) ? scale * W[i * in + k] : 0.f;
            const unsigned h16 = bf16_rne(v), l16 = bf16_rne(v - bf16_to_f32(h16));
            wh[t >> 1] |= h16 << (16 * (t & 1));
            wl[t >> 1] |= l16 << (16 * (t & 1));
        }
        frags[((net * 2 + 0) * nfw + f) * 64 + l] = frag_t{wh[0], wh[1], wh[2], wh[3]};
        frags[((net * 2 + 1) * nfw + f) * 64 + l] = frag_t{wl[0], wl[1], wl[2], wl[3]};
        return;
    }
    const int j = g - nfrag_thr;
    if (j < 2 * FWG_ACT_BIAS_FLOATS) {
        const int net = j / FWG_ACT_BIAS_FLOATS, c = j % FWG_ACT_BIAS_FLOATS;
        const int nout = net ? 1 : L.A;
        float v;
        if (c < 64) v = FWG_ACT_PRESCALE * params[L.b1[net] + c];
        else if (c < 128) v = FWG_ACT_PRESCALE * params[L.b2[net] + c - 64];
        else v = c - 128 < nout ? params[L.b3[net] + c - 128] : 0.f;
        bias[j] = v;
    } else if (j < 2 * FWG_ACT_BIAS_FLOATS + FWG_ACT_MAX_ACT) {
        const int a = j - 2 * FWG_ACT_BIAS_FLOATS;
        log_std[a] = a < L.A ? params[L.ls + a] : 0.f;
    } else if (L.cnn && j < 2 * FWG_ACT_BIAS_FLOATS + FWG_ACT_MAX_ACT + FWG_CNN_PARAMS) {
        const int i = j - 2 * FWG_ACT_BIAS_FLOATS - FWG_ACT_MAX_ACT;   // w[r][c] at r FILTERS + c, then b[c] (adjacent in the flat layout too)
        bias[2 * FWG_ACT_BIAS_FLOATS + i] = i < FWG_PPO_CNN_SUMS ? params[L.cw + i] : 0.f;
    }
}
