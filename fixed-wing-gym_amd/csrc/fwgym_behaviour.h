// fwgym_behaviour.h -- the behaviour policy of an off-policy learner on the device (fwg_behaviour_act; include/fwgym.h "Behaviour
// head"): what an exploration rollout for hindsight replay runs between two env steps, as ONE launch.
//
// A collection loop out of torch modules issues a cat, five Linear / activation launches, randn_like, a multiply-add, a clamp, three
// copies into rollout rows and a goal observation around every env step, and none of it can be captured: randn_like draws from the
// host generator and the step index is a Python integer.  k_behaviour_act composes what the other headers already hold --
// goal_rows_of (fwgym_goal.h: the code fwg_goal_observe runs), ddpg_gather / ddpg_forward<true> (fwgym_offpolicy.h: the actor's
// forward pass on a 64-row LDS tile, split-operand bf16 MFMA at fp32 accuracy), philox4x32 / box_muller -- per tile of 64 envs:
//   1. goal rows: with an env, the achieved / desired rows of the tile's envs -> achieved_out / desired_out (the rollout's goal log);
//      without one, goal_rows as given
//   2. [obs | goal] into the LDS tile (rows past N: zeros)
//   3. obs_out (if given) = the tile's observation rows: the rollout's obs[t], no copy launch
//   4. pi = tanh(actor([obs | goal])) from the flat parameter vector IN PLACE (the first PA words of the learner's online vector: an
//      update is seen by the next launch with no copy)
//   5. exploration, unless `deterministic`: c = draws[e], draws[e] = c + 1 (read and written by the env's own lane: nothing that
//      changes travels by value, so a captured launch replays correctly); with ctr = (env_id_base + e, c, sub, FWG_STREAM_BEHAVIOUR)
//      block sub 0 -> four normals n_i (box_muller), block sub 1 -> uniforms 2 u01(x_i) - 1, word 0 of block sub 2 < eps_scaled
//      decides: the uniform action, else clamp(pi_i + sigma n_i, -1, 1).  sigma and eps_scaled are read from noise_params (device
//      memory: a schedule changes them with one copy outside a graph)
//   6. action_out; done_out[e] = done_in[e] (if given): the act behind env step t files that step's done flags into dones[t]
// Every store is an ordinary vector store.  No atomics, no scratch, no spills.
#ifndef FWGYM_BEHAVIOUR_H
#define FWGYM_BEHAVIOUR_H

#define FWG_STREAM_BEHAVIOUR 12u          /* Philox stream of the exploration draws (1..11 are taken) */
#define FWG_BEHAVIOUR_NOISE_WORDS 4       /* noise_params: sigma (float bits), eps_scaled low word, eps_scaled high word (0 / 1), 0 */

struct BehaviourArgs {
    RecCfg rc;                    // (env launches) the arena's structure words, as fwg_goal_observe takes them
    GoalCfg g;
    const float* S;               // the env's arena, or null: goal rows are given
    long N;
    DdpgLayout L;                 // ddpg_layout(D, G, A, 1): the actor's segment is all that is read
    const float* params;          // [>= L.PA]
    const float* obs;             // [N][D]
    const float* goal_rows;       // [N][4] (no env), else null
    float4* achieved_out;         // [N] (env launches)
    float4* desired_out;
    float* obs_out;               // [N][D] or null
    float* action_out;            // [N][A]
    const unsigned char* done_in; // [N] or null
    unsigned char* done_out;
    unsigned* draws;              // [N] per-env draw counters
    const unsigned* noise_params; // [FWG_BEHAVIOUR_NOISE_WORDS]
    unsigned seed_lo, seed_hi, env_id_base;
    int deterministic;
};

__host__ __device__ inline int behaviour_lds_floats() { return 3 * FWG_PPO_ROWS * FWG_PPO_LS + 4 * FWG_PPO_ROWS; }

__global__ __launch_bounds__(FWG_PPO_THREADS) void k_behaviour_act(const BehaviourArgs B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LS = FWG_PPO_LS;
    const int tid = threadIdx.x;
    const DdpgLayout& L = B.L;
    float* Xs = lds;                        // [64][LS] [obs | goal]
    float* H1 = Xs + FWG_PPO_ROWS * LS;     // [64][LS] the actor's hidden layers
    float* H2 = H1 + FWG_PPO_ROWS * LS;
    float* pi = H2 + FWG_PPO_ROWS * LS;     // [64][4]
    const long r0 = (long)blockIdx.x * FWG_PPO_ROWS;
    const int nrows = (int)(B.N - r0 < FWG_PPO_ROWS ? B.N - r0 : FWG_PPO_ROWS);
    const bool mine = tid < nrows;          // this lane is env r0 + tid's own
    const long e = r0 + tid;
    const float* goal = B.goal_rows;
    if (B.S != nullptr) {
        if (mine) {
            float4 a, d;
            goal_rows_of(B.rc, B.g, B.S, B.N, e, a, d);
            B.achieved_out[e] = a;
            B.desired_out[e] = d;
        }
        goal = reinterpret_cast<const float*>(B.desired_out);
        __syncthreads();   // the tile's rows are read back below by other lanes of this workgroup
    }
    ddpg_gather(Xs, L, B.obs, goal, nullptr, r0, nrows, tid);
    __syncthreads();
    if (B.obs_out != nullptr) {
        for (int j = tid; j < nrows * L.D; j += FWG_PPO_THREADS) {
            const int r = j / L.D;
            B.obs_out[r0 * L.D + j] = Xs[r * LS + (j - r * L.D)];
        }
    }
    ddpg_forward<true>(B.params, L.actor, L.Ka, L.A, Xs, H1, H2, pi, tid);
    if (!mine) return;
    float act[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) act[i] = pi[tid * 4 + (i < L.A ? i : 0)];
    if (!B.deterministic) {
        const unsigned c = B.draws[e];
        B.draws[e] = c + 1u;
        const unsigned id = B.env_id_base + (unsigned)e;
        const float sigma = __uint_as_float(B.noise_params[0]);
        const unsigned long long eps_scaled = (unsigned long long)B.noise_params[1] | ((unsigned long long)B.noise_params[2] << 32);
        float n[4];
        box_muller(philox4x32(id, c, 0u, FWG_STREAM_BEHAVIOUR, B.seed_lo, B.seed_hi), n);
        const u4 ub = philox4x32(id, c, 1u, FWG_STREAM_BEHAVIOUR, B.seed_lo, B.seed_hi);
        const bool random = (unsigned long long)philox4x32(id, c, 2u, FWG_STREAM_BEHAVIOUR, B.seed_lo, B.seed_hi).x < eps_scaled;
        const float u[4] = {2.f * u01(ub.x) - 1.f, 2.f * u01(ub.y) - 1.f, 2.f * u01(ub.z) - 1.f, 2.f * u01(ub.w) - 1.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) act[i] = random ? u[i] : fminf(fmaxf(act[i] + sigma * n[i], -1.f), 1.f);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < L.A) B.action_out[e * L.A + i] = act[i];
    if (B.done_in != nullptr && B.done_out != nullptr) B.done_out[e] = B.done_in[e];
}

#endif /* FWGYM_BEHAVIOUR_H */
