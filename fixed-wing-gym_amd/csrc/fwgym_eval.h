// fwgym_eval.h -- the evaluation protocol on the device (fwg_pid_act, fwg_eval_advance; include/fwgym.h "Evaluation").
//
// The reference's evaluate_model_on_set (examples/evaluate_controller.py:44-169) flies every scenario of a test set to its FIRST
// episode end, feeds finished envs zero actions and keeps reward lists and the info dict of the step that ended each episode.
// Two kernels keep that loop off the host: the PID baseline's control law (pyfly.pid_controller.PIDController as
// gym_fixed_wing/pid.py BatchedPID restates it) and the tracker that folds one step's reward / done / metrics into per-scenario
// results.  Both are stateless launches over caller-owned buffers: one lane per env, guarded tail, no LDS, no atomics.
// Memory-trivial (tens of bytes per env and step), so the only thing that matters is that a wave's accesses fall into as few
// lines as possible: every per-env array is env-minor ([k][N]: 256-B row segments per wave), the observation / target rows are
// read where the env step left them (a wave touches 64 consecutive rows, every line of which it uses for several columns), and a
// 12-byte action row goes out as three stores into the wave's one 768-B span.
#ifndef FWGYM_EVAL_H
#define FWGYM_EVAL_H

#define FWG_EVAL_THREADS 256

struct PidCols { int roll, pitch, va, p, q, r, t_roll, t_pitch, t_va; };

// NaN-propagating clamp (torch.clamp's behaviour; fminf / fmaxf would turn a NaN into a limit)
__device__ __forceinline__ float pid_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// BatchedPID.get_action for N aircraft: roll PID on (phi, p) -> aileron, pitch PID on (theta, q rotated by roll) -> elevator, PI
// airspeed -> throttle.  The action comes from the integrals AS THEY STAND; dt * e is added to them afterwards.
// integ: [3][N] rows roll, pitch, Va.  act: [N][3] elevator, aileron, throttle.
__global__ __launch_bounds__(FWG_EVAL_THREADS) void k_pid_act(long N, const float* __restrict__ obs, int obs_stride, const float* __restrict__ target,
                                                               int target_stride, PidCols c, fwg_pid_gains g, float* __restrict__ integ,
                                                               float* __restrict__ act) {
    const long e = (long)blockIdx.x * FWG_EVAL_THREADS + threadIdx.x;
    if (e >= N) return;
    const float* o = obs + e * obs_stride;
    const float* tg = target + e * target_stride;
    const float phi = o[c.roll], theta = o[c.pitch], va = o[c.va];
    const float p = o[c.p], om_q = o[c.q], om_r = o[c.r];
    const float e_phi = phi - tg[c.t_roll], e_theta = theta - tg[c.t_pitch], e_va = va - tg[c.t_va];
    const float i_phi = integ[e], i_theta = integ[N + e], i_va = integ[2 * N + e];
    const float q = om_q * cosf(phi) - om_r * sinf(phi);
    const float delta_a = -g.k_p_phi * e_phi - g.k_i_phi * i_phi - g.k_d_phi * p;
    const float delta_e = -g.k_p_theta * e_theta - g.k_i_theta * i_theta - g.k_d_theta * q;
    const float delta_t = -g.k_p_V * e_va - g.k_i_V * i_va;
    integ[e] = i_phi + g.dt * e_phi;
    integ[N + e] = i_theta + g.dt * e_theta;
    integ[2 * N + e] = i_va + g.dt * e_va;
    act[3 * e] = pid_clamp(delta_e, g.delta_e_min, g.delta_e_max);
    act[3 * e + 1] = pid_clamp(delta_a, g.delta_a_min, g.delta_a_max);
    act[3 * e + 2] = pid_clamp(delta_t, g.delta_t_min, g.delta_t_max);
}

// The episode tracker, once per step t (after the controller, before the env step): folds step t - 1 (skipped at t == 0) and
// gates the actions of step t.  With auto_reset off a finished env keeps stepping and reports done again (the !c.auto_reset
// store of the episode-end block): `active` is what makes the FIRST end the one that is kept.
__global__ __launch_bounds__(FWG_EVAL_THREADS) void k_eval_advance(long N, long t, const float* __restrict__ reward, const unsigned char* __restrict__ done,
                                                                    const unsigned char* __restrict__ term, const float* __restrict__ metrics,
                                                                    unsigned char* __restrict__ active, int* __restrict__ length,
                                                                    unsigned char* __restrict__ termination, float* __restrict__ metrics_final,
                                                                    float* __restrict__ trace, float* __restrict__ actions) {
    const long e = (long)blockIdx.x * FWG_EVAL_THREADS + threadIdx.x;
    if (e >= N) return;
    bool on = active[e] != 0;
    if (t > 0) {
        if (on) {
            if (trace != nullptr) trace[(t - 1) * N + e] = reward[e];
            length[e] = (int)t;
            if (done[e]) {
                termination[e] = term[e];
                for (int k = 0; k < FWG_N_METRICS; ++k) metrics_final[k * N + e] = metrics[k * N + e];
                active[e] = 0;
                on = false;
            }
        } else if (trace != nullptr) trace[(t - 1) * N + e] = NAN;
    }
    // STORED, not multiplied: 0 * NaN is NaN, and a finished, tumbling aircraft's policy may well produce one
    if (actions != nullptr && !on) { actions[3 * e] = 0.f; actions[3 * e + 1] = 0.f; actions[3 * e + 2] = 0.f; }
}

#endif /* FWGYM_EVAL_H */
