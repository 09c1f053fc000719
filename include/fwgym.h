/*
 * fwgym.h -- C ABI of libfwgym.so, the MI355X-native batched replacement for the hot path
 *            FixedWingAircraft.step()/reset() of eivindeb/fixed-wing-gym.
 *
 * The reference has no FFI: its hot path is Python calling Python (gym_fixed_wing/fixed_wing.py calling
 * pyfly.pyfly.PyFly).  Each entry point below names the reference interface it replaces for a whole batch of
 * N independent environments ("one wavefront lane = one aircraft").  All pointers are DEVICE pointers unless the
 * parameter name ends in _host.  No torch types cross this boundary; `stream` is a hipStream_t passed as void*.
 *
 * Conventions
 *   - every function returns 0 on success or a negative fwg_status; fwg_last_error() gives the message
 *     (thread-local); nothing throws across the ABI.
 *   - per-environment SIMULATION failures are data, not API errors: done=1 and term_code=FWG_TERM_VAR0+var_id,
 *     mirroring fixed_wing.py:409-416.
 *   - the caller owns every buffer, including the persistent state arena (rows x N 32-bit words in 16-byte
 *     groups [rows/4][env][4]); the library allocates only its small device-side constant block and reduction scratch in
 *     fwg_create.  No allocation and no synchronisation happens in fwg_step/fwg_reset.
 *   - a handle is not thread-safe; use one handle per GPU/stream.
 */
#ifndef FWGYM_H
#define FWGYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FWG_ABI_VERSION 26

#define FWG_N_VARS 23        /* simulator variables, see fwg_var */
#define FWG_N_RESET_VARS 21  /* the keys of reset(state=...) records (fixed_wing.py:287,308; test-set format) */
#define FWG_N_PARAMS 49      /* aircraft parameters, see fwg_param */
#define FWG_MAX_OBS 32       /* observation.states entries per row (fixed_wing.py:796) */
#define FWG_MAX_ROWS 8       /* observation.length (fixed_wing.py:790) */
#define FWG_MAX_FACTORS 16   /* reward.factors (fixed_wing.py:683) */
#define FWG_MAX_TARGETS 3    /* target.states (fixed_wing.py:471) */
#define FWG_MAX_WINDOW 8     /* action window_size (fixed_wing.py:689,822) */
#define FWG_MAX_STREAK 128   /* target.success_streak_req (fixed_wing.py:377) */
#define FWG_END_WINDOW 50    /* end_error window (fixed_wing.py:1107) */
#define FWG_END_RING (FWG_END_WINDOW + 1)   /* slots of the cumulative-error ring: the window and the record just before it */
#define FWG_N_DRYDEN 8       /* Dryden filter states (joint realisation u | v,r | w,q | p) */
#define FWG_N_METRICS 28     /* rows of the metrics block written by fwg_step, see fwg_metric_row */
#define FWG_N_REDUCE 16      /* floats accumulated for fwg_reduce_success */
#define FWG_N_MONITOR 8      /* doubles written by fwg_monitor_take */

typedef enum fwg_status {
    FWG_OK = 0,
    FWG_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    FWG_ERR_ABI = -2,         /* struct size or version mismatch */
    FWG_ERR_HIP = -3,         /* a HIP runtime call failed */
    FWG_ERR_NAN_ACTION = -4   /* fwg_check_actions found NaN (reference: AssertionError, fixed_wing.py:347) */
} fwg_status;

/* simulator variable ids; 0..20 are exactly the keys of the reference's test-set "state" records */
typedef enum fwg_var {
    FWG_V_ROLL = 0, FWG_V_PITCH, FWG_V_YAW, FWG_V_OMEGA_P, FWG_V_OMEGA_Q, FWG_V_OMEGA_R,
    FWG_V_POS_N, FWG_V_POS_E, FWG_V_POS_D, FWG_V_VEL_U, FWG_V_VEL_V, FWG_V_VEL_W,
    FWG_V_VA, FWG_V_ALPHA, FWG_V_BETA, FWG_V_ELEVATOR, FWG_V_AILERON, FWG_V_THROTTLE,
    FWG_V_WIND_N, FWG_V_WIND_E, FWG_V_WIND_D, FWG_V_ELEVON_RIGHT, FWG_V_ELEVON_LEFT
} fwg_var;

/* aircraft parameter ids (names of the X8 parameter table, simulator.params[name] at fixed_wing.py:539) */
typedef enum fwg_param {
    FWG_P_MASS = 0, FWG_P_JX, FWG_P_JY, FWG_P_JZ, FWG_P_JXZ, FWG_P_S_WING, FWG_P_B, FWG_P_C, FWG_P_S_PROP,
    FWG_P_C_PROP, FWG_P_K_MOTOR, FWG_P_K_T_P, FWG_P_K_OMEGA, FWG_P_E, FWG_P_AR, FWG_P_M, FWG_P_A_0,
    FWG_P_C_LIFT_0, FWG_P_C_LIFT_ALPHA, FWG_P_C_LIFT_Q, FWG_P_C_LIFT_DELTA_E, FWG_P_C_D_P, FWG_P_C_D_BETA1, FWG_P_C_D_BETA2,
    FWG_P_C_D_Q, FWG_P_C_D_DELTA_E, FWG_P_C_M_0, FWG_P_C_M_ALPHA, FWG_P_C_M_Q, FWG_P_C_M_DELTA_E, FWG_P_C_M_FP,
    FWG_P_C_Y_0, FWG_P_C_Y_BETA, FWG_P_C_Y_P, FWG_P_C_Y_R, FWG_P_C_Y_DELTA_A, FWG_P_C_Y_DELTA_R,
    FWG_P_C_ROLL_0, FWG_P_C_ROLL_BETA, FWG_P_C_ROLL_P, FWG_P_C_ROLL_R, FWG_P_C_ROLL_DELTA_A, FWG_P_C_ROLL_DELTA_R,
    FWG_P_C_N_0, FWG_P_C_N_BETA, FWG_P_C_N_P, FWG_P_C_N_R, FWG_P_C_N_DELTA_A, FWG_P_C_N_DELTA_R
} fwg_param;

/* termination codes written to term_code_out (info["termination"], fixed_wing.py:368,385,416) */
enum {
    FWG_TERM_NONE = 0,
    FWG_TERM_STEPS = 1,      /* "steps"   */
    FWG_TERM_SUCCESS = 2,    /* "success" */
    FWG_TERM_VAR0 = 16,      /* FWG_TERM_VAR0 + fwg_var = name of the violated simulator variable */
    FWG_TERM_NAN = 255       /* a state became non-finite */
};

/* observation.states[i] (fixed_wing.py:796-838) */
enum { FWG_OBS_STATE = 0, FWG_OBS_TARGET_RELATIVE = 1, FWG_OBS_TARGET_ABSOLUTE = 2, FWG_OBS_ACTION = 3,
       FWG_OBS_TARGET_INTEGRATOR = 4 /* windowed error sum over integration_window steps (fixed_wing.py:804-810) */ };
typedef struct fwg_obs_desc {
    int32_t type;      /* FWG_OBS_* */
    int32_t src;       /* STATE: fwg_var; TARGET_*: index into target.states; ACTION: index into action.states */
    int32_t window;    /* ACTION: window_size (fixed_wing.py:822) */
    int32_t norm;      /* apply (val-mean)/var (fixed_wing.py:833-835) */
    double mean;
    double var;        /* the reference divides by "var" itself */
} fwg_obs_desc;

/* target.states[i] (fixed_wing.py:461-521, 933-991) */
enum { FWG_TGT_CONSTANT = 0, FWG_TGT_COMPENSATE = 1, FWG_TGT_LINEAR = 2, FWG_TGT_SINUSOIDAL = 3 };
typedef struct fwg_target_desc {
    int32_t var;       /* fwg_var */
    int32_t cls;       /* FWG_TGT_* */
    int32_t wrap;      /* simulator.state[name].wrap (fixed_wing.py:897,988) */
    int32_t has_delta;
    int32_t has_bound;
    int32_t pad_;
    double low, high;  /* radians where convert_to_radians; AFTER curriculum scaling (fixed_wing.py:256-265) */
    double delta;
    double bound;
    double slope_low, slope_high;          /* LINEAR (radians/s where flagged) */
    double amplitude_low, amplitude_high;  /* SINUSOIDAL */
    double period_low, period_high;
} fwg_target_desc;

/* reward.factors[i] (fixed_wing.py:683-751) */
enum { FWG_RC_STATE = 0, FWG_RC_ACTION = 1, FWG_RC_SUCCESS = 2, FWG_RC_STEP = 3, FWG_RC_GOAL = 4 };
enum { FWG_RT_VALUE = 0, FWG_RT_ERROR = 1, FWG_RT_DELTA = 2, FWG_RT_BOUND = 3, FWG_RT_PER_STATE = 4, FWG_RT_ALL = 5,
       FWG_RT_INT_ERROR = 6 /* fixed_wing.py:708-711 */ };
enum { FWG_FC_LINEAR = 0, FWG_FC_QUADRATIC = 1, FWG_FC_EXPONENTIAL = 2 };
typedef struct fwg_factor_desc {
    int32_t cls;       /* FWG_RC_* */
    int32_t type;      /* FWG_RT_* */
    int32_t src;       /* STATE/VALUE: fwg_var; STATE/ERROR: target index */
    int32_t fclass;    /* FWG_FC_* */
    int32_t shaping;
    int32_t window;    /* ACTION/DELTA */
    int32_t has_max;
    int32_t value_is_timesteps;  /* SUCCESS with value "timesteps" (fixed_wing.py:716) */
    double sign;       /* np.sign(sign) */
    double scaling;
    double max;
    double value;
} fwg_factor_desc;

enum { FWG_TURB_FILTER = 0, FWG_TURB_INCREMENT = 1 };
enum { FWG_ON_SUCCESS_NONE = 0, FWG_ON_SUCCESS_DONE = 1, FWG_ON_SUCCESS_NEW = 2 };

/* Flat, host-side "compiled" form of fixed_wing_config.json + the simulator config + the aircraft parameter table.
 * Angles are radians.  +-INFINITY encodes an absent min/max. */
typedef struct fwg_config {
    uint32_t abi_version;   /* FWG_ABI_VERSION */
    uint32_t struct_bytes;  /* sizeof(fwg_config) as seen by the caller */

    /* ---- simulator (replaces the PyFly object built at fixed_wing.py:41-46) */
    double dt, rho, g;
    int32_t n_substeps;     /* RK4 steps of the 13 rigid-body states per env step */
    int32_t actuator_microsteps; /* exact actuator micro-steps per env step (multiple of 2*n_substeps) */
    int32_t turbulence;     /* sim_config_kw["turbulence"] (examples/evaluate_controller.py:78) */
    int32_t turbulence_output;  /* FWG_TURB_INCREMENT (default of sim_config.json) | FWG_TURB_FILTER: what enters the airspeed and
                                 * body rates -- the first difference of the Dryden filter outputs (PyFly 0.1.2 as observed in
                                 * the reference's published traces) or the MIL-F-8785C outputs themselves */
    double param[FWG_N_PARAMS];
    double con_min[FWG_N_VARS], con_max[FWG_N_VARS];    /* Variable.constraint_min/max  */
    double val_min[FWG_N_VARS], val_max[FWG_N_VARS];    /* Variable.value_min/max       */
    double init_min[FWG_N_VARS], init_max[FWG_N_VARS];  /* Variable.init_min/max AFTER curriculum (fixed_wing.py:233-245) */
    double elevon_omega0[2], elevon_zeta[2], elevon_dot_max[2];  /* [right, left] */
    double throttle_tau;
    double dryden_A[FWG_N_DRYDEN * FWG_N_DRYDEN];  /* discrete x' = A x + B n, row-major */
    double dryden_B[FWG_N_DRYDEN * 4];             /* includes the sqrt(pi/dt) white-noise scaling */
    double dryden_C[6 * FWG_N_DRYDEN];             /* gust (u,v,w,p,q,r) = C x */

    /* ---- gym side */
    int32_t steps_max;                  /* fixed_wing.py:49 */
    int32_t obs_length, obs_step;       /* fixed_wing.py:786-790 */
    int32_t n_obs;                      /* len(observation.states) */
    int32_t obs_normalize;              /* fixed_wing.py:59 */
    int32_t obs_noise;                  /* observation.noise present with var != 0 or mean != 0 */
    double obs_noise_mean, obs_noise_std;
    fwg_obs_desc obs[FWG_MAX_OBS];

    int32_t n_actions;                  /* must be 3: elevator, aileron, throttle */
    int32_t scale_actions;              /* action.scale_space (fixed_wing.py:185,349) */
    double scale_low, scale_high;
    double act_to_low[3], act_to_high[3];      /* action_scale_to_low/high (fixed_wing.py:177-178) */
    int32_t has_action_bounds, pad0_;
    double act_bound_min[3], act_bound_max[3]; /* fixed_wing.py:187-191 */

    int32_t n_targets, resample_every, streak_req, on_success;  /* fixed_wing.py:377-398 */
    double streak_fraction;
    fwg_target_desc target[FWG_MAX_TARGETS];

    int32_t reward_potential;           /* reward.form == "potential" */
    int32_t step_fail_timesteps;        /* reward.step_fail == "timesteps" (fixed_wing.py:411-415) */
    double step_fail_value;
    int32_t term_present[3];            /* reward.terms by FWG_FC_* */
    int32_t n_factors;
    double term_weight[3];
    fwg_factor_desc factor[FWG_MAX_FACTORS];

    int32_t metrics;                    /* any entry in cfg["metrics"] (fixed_wing.py:419-421) */
    int32_t auto_reset;                 /* VecEnv semantics: a done env restarts inside the same fwg_step */
    int32_t store_derived;              /* keep roll/pitch/yaw/Va/alpha/beta of the committed state in the arena (host views) */
    int32_t obs_log_rows;   /* 0: fwg_step writes the dense [N][obs_dim] batch.  L > 0 (matrix observations without
                             * observation noise): observation history kept once, as a row log -- see fwg_obs_window */
    double rise_low, rise_high;         /* metrics[rise_time].low/high (fixed_wing.py:1131) */

    /* ---- simulator["model"]: aircraft parameters re-sampled for every env at every reset (sample_simulator_parameters,
     * fixed_wing.py:532-559).  Listed parameter i has id model_idx[i]; its nominal value is param[id].  Gaussian:
     * N(nominal, model_var[i]) then min(max(x, model_clip_lo[i]), model_clip_hi[i]) (-/+INFINITY = no clip; numpy's clip
     * order, so an interval given upside down -- relative clip of a negative nominal -- collapses to its upper end).
     * Uniform: U(nominal - model_var[i], nominal + model_var[i]).  Entries with nominal == 0 are skipped by the caller. */
    int32_t model_n;                    /* 0 = off */
    int32_t model_dist;                 /* 0 gaussian, 1 uniform */
    int32_t model_idx[FWG_N_PARAMS];
    int32_t pad_model_;
    double model_var[FWG_N_PARAMS], model_clip_lo[FWG_N_PARAMS], model_clip_hi[FWG_N_PARAMS];

    /* ---- reward["randomize_scaling"] (fixed_wing.py:330-334): factors whose scaling is given as [low, high] get a
     * scaling drawn U(low, high) for every env at every reset; low == high: the fixed factor[i].scaling */
    int32_t randomize_scaling;
    int32_t integration_window;  /* fixed_wing.py:53: window of the integrator observations / int_error factors (0: none; <= FWG_END_WINDOW - 1) */
    /* ---- simulator.<key> sampling at every reset (fixed_wing.py:560-569) for the two turbulence keys.  Per env and episode the
     * gust is scaled by on(turbulence) * W20(turbulence_intensity) / W20(the intensity dryden_C was built for): the intensity
     * only enters the MIL-F-8785C filters as an output gain.  n = 0: the key is not sampled (the configuration's value holds). */
    int32_t sk_n_intensity, sk_n_turbulence;
    int32_t sk_index_intensity, sk_index_turbulence;   /* position among the sampled keys (RNG sub-stream) */
    double sk_cum_intensity[4], sk_gain_intensity[4];  /* cumulative probabilities / gain of each listed value */
    double sk_cum_turbulence[2], sk_on_turbulence[2];
    double sk_base_gain;                               /* gain of the keys that are not sampled (0 when turbulence is configured off) */
    double factor_scaling_low[FWG_MAX_FACTORS], factor_scaling_high[FWG_MAX_FACTORS];
} fwg_config;

/* The caller-owned state arena is an array of 16-byte GROUPS [rows/4][N] of 32-bit words: word w of env e lives at
 * ((w >> 2) * N + e) * 4 + (w & 3).  All offsets below are in words and multiples of 4. */
typedef struct fwg_layout {
    int32_t rows;        /* total words per env (multiple of 4); arena = rows * N words */
    int32_t sim;         /* 28: e0 e1 e2 e3 | p q r pn | pe pd u v | w elevon_r elevon_l throttle | elevon_r_dot elevon_l_dot dryden0 dryden1 | dryden2..5 | dryden6 dryden7 pad pad */
    int32_t cold;        /* 8: wind_n wind_e wind_d episode | e0(3) pad -- per-episode constants, written by reset only */
    int32_t derived;     /* 8: roll pitch yaw Va | alpha beta pad pad of the committed state (written when store_derived) */
    int32_t gym;         /* 36: tgt0 tgt1 tgt2 steps_count|steps_for_target<<16 | flags window_counts goal_counts(2) | prev_cmd(3) sum_dcmd | settle(2) rise0 rise1 | rise2 sum_e(3) | sum_abs_e(3) prev_err0 | min_e(3) prev_err1 | max_e(3) prev_err2 | prev_shaping(3) pad */
    int32_t tprop;       /* 12: per target slope|amplitude, period, phase, bias (linear/sinusoidal targets) */
    int32_t goal;        /* 16 plain word rows [word][N] (NOT grouped): goal-window ring, 8 positions x 4 flags per word */
    int32_t act_ring;    /* window*4: raw actions (a0 a1 a2 pad) per slot, slot = global_step % window */
    int32_t cmd_ring;    /* window*4: constrained commands (only when observations need them) */
    int32_t end_ring;    /* 51*4: cumulative error sums of the episode (S0 S1 S2 pad) per slot, slot = global_step % 51 */
    int32_t lag_ring;    /* lag_depth*lag_groups*4: normalised observation records, slot = global_step % lag_depth */
    int32_t window;      /* action window depth */
    int32_t lag_depth;   /* (length-1)*step+1 */
    int32_t lag_groups;  /* ceil(n_obs/4) */
    int32_t draw;        /* 44 (+12 with linear/sinusoidal targets): the NEXT episode's reset draw, prepared ahead of time (cold) */
    int32_t aero;        /* 52 (model randomisation only): this episode's 49 force/moment constants of the env | - - - */
    int32_t aero_next;   /* 52: the next episode's | episode it is for, configuration generation, - */
    int32_t fscale;      /* 16 (reward.randomize_scaling only): 1 / scaling of every reward factor, this episode */
    int32_t fscale_next; /* 20: the next episode's | episode it is for, configuration generation, - - */
    int32_t model_raw;      /* model_n rounded up to 4: the sampled values of the listed parameters, this episode (get_simulator_parameters, fixed_wing.py:872-888) */
    int32_t model_raw_next; /* the same for the next episode (validity: the tag of aero_next) */
    int32_t fin;         /* 28 (metrics only): the raw accumulators of the env's last finished episode, turned into the metrics
                          * block and the success sums by fwg_finish_episodes / fwg_reduce_success* (flag bit 7 of the flags word) */
} fwg_layout;

/* rows of the metrics block (float32 [FWG_N_METRICS][N], valid where done) -- get_metric, fixed_wing.py:1095-1162 */
typedef enum fwg_metric_row {
    FWG_M_RISE_TIME = 0,          /* 3 */
    FWG_M_SETTLING_TIME = 3,      /* 4: target0..2, all */
    FWG_M_OVERSHOOT = 7,          /* 3 */
    FWG_M_TOTAL_ERROR = 10,       /* 3 */
    FWG_M_AVG_ERROR = 13,         /* 3 */
    FWG_M_CONTROL_VARIATION = 16, /* 1 */
    FWG_M_SUCCESS = 17,           /* 4 */
    FWG_M_SUCCESS_TIME_FRAC = 21, /* 4 */
    FWG_M_END_ERROR = 25          /* 3 */
} fwg_metric_row;

typedef struct fwg_handle fwg_handle;

/* Library/ABI version check. */
int fwg_abi_version(void);

/* Computes the arena layout for a configuration (pure host function). */
int fwg_get_layout(const fwg_config* cfg_host, fwg_layout* out_host);

/* Replaces FixedWingAircraft.__init__ (fixed_wing.py:14-212) for n_envs environments on HIP device `device`.
 * `state_arena` must hold layout.rows * n_envs 32-bit words (16-byte aligned, zero-initialised) and stay alive until
 * fwg_destroy.
 * `env_id_base` is the global index of this handle's first env (multi-GPU sharding: RNG streams depend only on the
 * global env index, so results do not depend on how envs are split over GPUs). */
int fwg_create(const fwg_config* cfg_host, int64_t n_envs, int device, void* state_arena, int64_t env_id_base,
               fwg_handle** out);
int fwg_destroy(fwg_handle* h);

/* Re-uploads the constants after a host-side change that keeps the layout (set_curriculum_level, fixed_wing.py:224-285;
 * setattr(simulator, key, val), fixed_wing.py:570). */
int fwg_update_config(fwg_handle* h, const fwg_config* cfg_host);

/* FixedWingAircraft.seed (fixed_wing.py:214-222): key of the counter-based device RNG. */
int fwg_seed(fwg_handle* h, uint64_t seed);

/* FixedWingAircraft.reset (fixed_wing.py:287-336) for the envs selected by `mask` (NULL = all).
 *   init_state : NULL or float32 [FWG_N_RESET_VARS][N]; NaN entries are sampled from init_min/init_max
 *                (reset(state=...) semantics, fixed_wing.py:308)
 *   init_target: NULL or float32 [n_targets][N]; NaN entries are sampled (reset(target=...), fixed_wing.py:311-315)
 *   obs_out    : float32 [N][obs_length*n_obs]; rows of unselected envs are left untouched */
int fwg_reset(fwg_handle* h, const uint8_t* mask, const float* init_state, const float* init_target,
              float* obs_out, void* stream);

/* FixedWingAircraft.step (fixed_wing.py:338-437) for all N envs, one fused launch.
 *   actions          : float32 [N][3] raw policy actions
 *   obs_out          : float32 [N][obs_length*n_obs]
 *   reward_out       : float32 [N]
 *   done_out         : uint8 [N]
 *   term_code_out    : uint8 [N]  FWG_TERM_*
 *   terminal_obs_out : NULL or float32 [N][obs_dim]; written for done envs only (VecEnv "terminal_observation")
 *   metrics_out      : NULL or float32 [FWG_N_METRICS][N]; written for done envs, by the NEXT fwg_finish_episodes /
 *                      fwg_reduce_success* call (the step itself only records the episode's accumulators).  LIFETIME: the
 *                      pointer of the LAST fwg_step is remembered and written through by fwg_reduce_success* -- keep the
 *                      buffer alive (or pass the same one every step) until the next collection; readers on the device
 *                      must order themselves after fwg_finish_episodes, not after fwg_step.  An env that ends two episodes
 *                      between collections keeps only the later one's column (both count in the success sums)
 *   target_out       : NULL or float32 [N][n_targets] = info["target"] (fixed_wing.py:435) after the step */
int fwg_step(fwg_handle* h, const float* actions, float* obs_out, float* reward_out, uint8_t* done_out,
             uint8_t* term_code_out, float* terminal_obs_out, float* metrics_out, float* target_out, void* stream);

/* Row-log observations (fwg_config.obs_log_rows = L > 0).  A lagged observation matrix is the newest record on top of
 * records the env already produced obs_step, 2 obs_step, ... steps ago; instead of copying those rows into a dense
 * batch every step (80 % of the observation traffic), fwg_step appends the new record to a log laid out as
 * float32 [obs_step][L][N][n_obs] -- the buffer passed as obs_out to fwg_reset / fwg_step, fwg_obs_log_floats() long --
 * in DESCENDING row order, so that the current observation of env e is the strided window
 *     obs[e][i][k] = log[((*plane + i) * N + e) * n_obs + k],  i < obs_length
 * (a zero-copy view: torch `log.view(-1, N, n_obs)[plane : plane + length].permute(1, 0, 2)`), valid until the next
 * fwg_step / fwg_reset.  Values are identical to the dense batch.  `plane` refers to the last completed step. */
int64_t fwg_obs_log_floats(const fwg_config* cfg_host, int64_t n_envs);
int fwg_obs_window(const fwg_handle* h, int64_t* plane);
/* Dense copy [N][obs_length * n_obs] of the current window of `obs_log` (the buffer fwg_step writes), for consumers that
 * need contiguous rows.  Stream-ordered; in graph mode the window position is read on the DEVICE, so the call may be
 * captured and replayed (a host-side view from fwg_obs_window is only valid for direct calls).  n_obs % 4 == 0. */
int fwg_obs_gather(const fwg_handle* h, const float* obs_log, float* obs_out, void* stream);

/* Known-answer hook: runs the device's Philox4x32-10 (the generator behind every sampled reset state, target, noise
 * and turbulence sample) on n inputs {counter[4], key[2]} (uint32 [n][6], device) -> uint32 [n][4] (device), so that
 * tests can check it against the published Random123 vectors.  Not used by the product path. */
int fwg_selftest_philox(const uint32_t* ctr_key_dev, uint32_t* out_dev, int64_t n, void* stream);

/* Debug-mode check for NaN actions (fixed_wing.py:347); synchronises the stream. */
int fwg_check_actions(fwg_handle* h, const float* actions, void* stream);

/* Local sums over the episodes finished since the last call: out_host[0]=episodes, [1..4]=success target0..2/all,
 * [5]=sum control_variation, [6..8]=sum end_error, [9..11]=sum total_error, [12..15]=sum success_time_frac.
 * These are the per-GPU contributions to the curriculum/logging reduction of
 * examples/train_rl_controller.py:51-66,80-85; the caller all-gathers them over RCCL.  Synchronises the stream and
 * clears the accumulators. */
int fwg_reduce_success(fwg_handle* h, float* out_host, void* stream);
/* Episode ends are recorded by fwg_step as a compact per-env record; THIS call (one small launch, stream-ordered, no
 * synchronisation) turns the records not yet collected into the metrics block (metrics_out: NULL or float32
 * [FWG_N_METRICS][N], written for the envs collected) and adds them to the success sums.  fwg_reduce_success and
 * fwg_reduce_success_device collect first (with the metrics_out of the last fwg_step).  Call it before reading the metrics of
 * the envs a step reported done; an env that ends a second episode before any collection folds the first record itself. */
int fwg_finish_episodes(fwg_handle* h, float* metrics_out, void* stream);
/* The same sums into a DEVICE buffer (16 floats), stream-ordered and without synchronising: the form to hand to the
 * RCCL all-gather directly, so that the rollout never drains the GPU for the success reduction. */
int fwg_reduce_success_device(fwg_handle* h, float* out_dev, void* stream);

/* Build-time specialisation support: writes the lowered STATIC configuration as 32-bit words (pure host function; the
 * build freezes such word lists into constexpr objects, see csrc/fwgym.hip "Specialisation").  Returns the number of
 * words, or a negative fwg_status. */
int fwg_dump_spec(const fwg_config* cfg_host, uint32_t* words_out_host, int64_t capacity);
/* Number of frozen configurations compiled into this library, and the kernel instance a handle runs: -1 = the generic
 * kernel (configuration interpreted at run time), i in [0, fwg_num_specs()) = frozen configuration i, FWG_INSTANCE_SHAPE + i =
 * the SHAPE instance of frozen configuration i -- the same structure (every count, type, source, flag: the integer members of
 * the lowered configuration) with the configuration's own VALUES (reward scalings, normalisation, constraints, aircraft
 * constants, noise levels, the time limit ...) read from memory: what a configuration that differs from a frozen one in values
 * only runs without any run-time compilation, ~1.1x the frozen kernel's step time (the generic kernel: ~35x). */
int fwg_num_specs(void);
int fwg_spec_index(const fwg_handle* h);
#define FWG_INSTANCE_SHAPE 1000
#define FWG_INSTANCE_GENERIC 100000
/* The instance fwg_create would pick for this configuration (pure host function): as fwg_spec_index, but FWG_INSTANCE_GENERIC
 * for the generic kernel, so that negative values stay fwg_status codes.  Replaces nothing in the reference (its env is
 * interpreted Python throughout); lets a host decide whether compiling a specialised kernel at run time is worth it. */
int fwg_config_instance(const fwg_config* cfg_host);

/* hipGraph support.  The ring positions of a launch depend on the global step counter; in graph mode that counter
 * lives on the device (each step launch publishes counter+1), so a captured sequence of fwg_step launches can be
 * replayed any number of times.  Rules: enable before capturing; capture an EVEN number of fwg_step calls per graph
 * (the counter is double-buffered by parity); after every replay tell the host how many steps ran
 * (fwg_note_replayed_steps) before issuing further direct calls.  Both functions synchronise `stream`/are host-only. */
int fwg_set_graph_mode(fwg_handle* h, int enable, void* stream);
int fwg_capture_begin(fwg_handle* h);   /* bracket the fwg_step calls issued under stream capture (they do not execute) */
int fwg_capture_end(fwg_handle* h);
int fwg_note_replayed_steps(fwg_handle* h, int64_t n_steps);
/* A captured sequence has the double-buffer copy its first launch reads baked in: it may only be replayed when the step
 * counter has the parity it had at fwg_capture_begin.  fwg_capture_parity: that parity (0 / 1) for the capture just
 * bracketed; fwg_replay_check: FWG_ERR_INVALID unless the handle's current step count has parity `capture_parity` -- call
 * it before every replay (host-only, no synchronisation).  With simulator.model / reward.randomize_scaling the captured
 * sequence is also tied to the configuration generation: fwg_capture_begin fails while every per-env parameter set is stale
 * (right after fwg_create / fwg_update_config / fwg_seed: issue fwg_reset or two direct steps first) and fwg_replay_check
 * fails for a sequence captured before the last fwg_update_config / fwg_seed (capture again). */
int fwg_capture_parity(const fwg_handle* h);
int fwg_replay_check(const fwg_handle* h, int capture_parity);


/* ---------------------------------------------------------------------------------------------------------------------
 * Rollout head ("actor"): what sits between two env steps in the reference's training/evaluation loops --
 * VecNormalize (running observation / return normalisation) around the env and the stable-baselines MlpPolicy
 * (pi and vf: obs -> 64 tanh -> 64 tanh -> act_dim / 1, state-independent log-std) acting on the normalised
 * observation (examples/train_rl_controller.py:223-231, examples/evaluate_controller.py:93-100) -- as two HIP kernels
 * on device-resident batches, so that one rollout step is three launches (fwg_step, fwg_actor_observe, fwg_actor_act).
 * The MLP runs on the matrix cores (bf16 MFMA, each fp32 operand split into bf16 hi + lo: three products per tile), weights
 * resident in LDS.  Precision of the split products, measured per element against float64 over obs_dim 1..64, act_dim 1..4 with
 * weights that take tanh out of its linear range: mean and value within 3.7e-5 of max(|result|, 1) on the host emulation of the
 * kernels, 4.9e-5 end to end for one-row batches (see fwg_actor_observe); profiles/actor_contract_errors.txt holds the tables per
 * shape and machine (fp32 torch on the same inputs: 9e-7).  tests/test_actor_contract.py asserts twice the worst measured figure,
 * and never more than 1e-4: one of the three products lost costs ~2^-9 of a term.  Single products (precise = 0): ~5e-3 of the
 * largest output.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fwg_actor fwg_actor;

/* Row-major float32 host arrays in torch.nn.Linear layout (weight [out][in], bias [out]); hidden width is 64.  A CNN head
 * (fwg_actor_set_conv) takes the conv's n_filters x features outputs in layer 0: pi_w0 / vf_w0 are [64][n_filters * features]. */
typedef struct fwg_actor_weights {
    const float *pi_w0, *pi_b0, *pi_w1, *pi_b1, *pi_w2, *pi_b2;   /* [64][obs_dim],[64],[64][64],[64],[act_dim][64],[act_dim] */
    const float *vf_w0, *vf_b0, *vf_w1, *vf_b1, *vf_w2, *vf_b2;   /* ... [1][64],[1] */
    const float *log_std;                                          /* [act_dim] */
} fwg_actor_weights;

/* Running statistics as VecNormalize keeps them (obs_rms, ret_rms). */
typedef struct fwg_actor_stats {
    float obs_mean[64], obs_var[64];
    float obs_count, ret_mean, ret_var, ret_count;
} fwg_actor_stats;

/* obs_dim <= 64 (a matrix observation is taken flattened), act_dim <= 4.  gamma/clip/epsilon: VecNormalize arguments
 * (defaults of the reference's scripts: 0.99, 10, 10, 1e-8). */
int fwg_actor_create(int device, int64_t n_envs, int obs_dim, int act_dim, float gamma, float clip_obs,
                     float clip_reward, float epsilon, fwg_actor** out);
void fwg_actor_destroy(fwg_actor* a);
int fwg_actor_set_weights(fwg_actor* a, const fwg_actor_weights* w_host);
/* CNN front end: the CnnMlpPolicy of the reference's CNN controller (examples/train_rl_controller.py:179-197, --policy CNN;
 * shipped as examples/models/cnn_controller, policy_kwargs {n_filters: 3}, observation Box(5, 12)).  The normalised observation,
 * taken as `rows` x features (features = obs_dim / rows, row-major: VecNormalize's order and the env's row log), passes one
 * VALID conv whose kernel spans the whole window and one feature (output height 1), shared by pi and vf:
 *     y[j][c] = tanh(b[c] + sum_r w[r][c] x[r][j]),  layer 0 input k = j * n_filters + c  (TF's NHWC flatten)
 * w [rows][n_filters] (the TF kernel [rows][1][1][n_filters]), b [n_filters]; then fwg_actor_set_weights with [64][n_filters *
 * features] layer-0 weights.  Refused (FWG_ERR_INVALID, fwg_last_error): non-matrix observations (rows < 2 or obs_dim not a
 * multiple of rows), rows other than the observation length of the row log set with fwg_actor_set_obs_log (the conv spans the
 * whole window), n_filters x features > 64, and any geometry other than 5 x 12 x 3 filters (the kernel instance of this build).
 * n_filters = 0 switches back to the MLP on the flattened observation.  fwg_rollout_available() is 0 for a CNN head (the
 * one-launch step runs the MLP head only) and fwg_learner_create refuses it (no backward pass through the conv). */
int fwg_actor_set_conv(fwg_actor* a, int n_filters, int rows, const float* w_host, const float* b_host);
int fwg_actor_set_stats(fwg_actor* a, const fwg_actor_stats* s_host, void* stream);
int fwg_actor_get_stats(fwg_actor* a, fwg_actor_stats* s_host, void* stream);   /* synchronises the stream */
/* training != 0: fwg_actor_act folds the batches seen by fwg_actor_observe into the running statistics (VecNormalize
 * training mode); 0: statistics frozen (evaluation).  precise != 0 (default): split-bf16 products; 0: plain bf16. */
int fwg_actor_configure(fwg_actor* a, int training, int precise);
/* Sampling noise: Philox stream (seed, env_id_base + env, act counter). */
int fwg_actor_seed(fwg_actor* a, uint64_t seed, int64_t env_id_base);
/* Attaches the head to an env (NULL detaches): from then on every fwg_step also leaves the batch moments of the
 * observations it writes and advances the discounted returns with the rewards it writes -- what fwg_actor_observe
 * would do in a launch of its own -- so that a rollout step is two launches (fwg_step, fwg_actor_act).  Same n_envs,
 * obs_dim and device required.  The env keeps a plain pointer: detach (or destroy the env) before fwg_actor_destroy. */
int fwg_attach_observer(fwg_handle* h, fwg_actor* a);
/* Row-log observations: after this call the `obs` argument of fwg_actor_observe / fwg_actor_act is `env`'s observation
 * row log and the head reads the window of the env's last completed step out of it (strided, no dense copy; position
 * taken from the host count for direct calls and from the device-resident positions in graph mode, so captured
 * sequences replay correctly).  NULL switches back to dense [N][obs_dim] batches.  The head keeps a plain pointer. */
int fwg_actor_set_obs_log(fwg_actor* a, const fwg_handle* env);
/* Accumulates the batch moments of `obs` ([N][obs_dim]) and, when `reward` is not NULL, advances the discounted
 * returns (ret = ret * gamma + reward, zeroed where `done`) and accumulates their moments (VecNormalize.step_wait).
 * Conditioning: the moments are sums of deviations from the running mean as it stood at the last fwg_actor_act (0 before the
 * first), folded in fp32 as s2 - s1^2, so the relative error of the running variance grows with the square of the distance
 * between a batch's mean and that running mean, in units of the batch's standard deviation:
 *     <= 8 * 2^-24 * (1 + (mean / std)^2)   -- 4.8e-5 at a ratio of 10, 4.8e-3 at 100
 * (the running mean itself stays within 2e-5).  The reference's VecNormalize is float64 and has no such limit; this env's
 * observations stay below a ratio of about 10.  The batch sums travel as fixed-point integers of quantum 2^-20, which shows only
 * for batches of a few rows: the mean of a one-row batch is off by up to 2^-21. */
int fwg_actor_observe(fwg_actor* a, const float* obs, const float* reward, const uint8_t* done, void* stream);
/* Folds the accumulated moments into the running statistics (training mode), normalises `obs`, evaluates pi and vf,
 * samples the action (or takes the mean when deterministic != 0).  Outputs (each may be NULL):
 *   norm_obs_out [N][obs_dim], action_out [N][act_dim], value_out [N], logp_out [N],
 *   norm_reward_out [N] = clip(reward / sqrt(ret_var + eps)) for the `reward` given (the transition that led here),
 *   done_out [N] = copy of `done` (so that a rollout buffer is filled without extra copy launches).
 * Launches under stream capture must come in EVEN numbers per graph (the statistics are double-buffered by parity). */
int fwg_actor_act(fwg_actor* a, const float* obs, const float* reward, const uint8_t* done, float* norm_obs_out,
                  float* action_out, float* value_out, float* logp_out, float* norm_reward_out, uint8_t* done_out,
                  int deterministic, void* stream);

/* One rollout step in ONE launch: the head on the observation the env currently shows, then the env step under the actions
 * just sampled -- the body of the reference's training loop, VecNormalize(SubprocVecEnv).step_wait inside PPO2's runner
 * (examples/train_rl_controller.py:223-231), without a launch boundary between policy and env.  Equivalent to
 *     fwg_actor_act(head, obs_io, reward_io, done_io, norm_obs_out, action_out, value_out, logp_out, norm_reward_out,
 *                   done_prev_out, deterministic, stream);
 *     fwg_step(env, action_out, obs_io, reward_io, done_io, term_code_out, terminal_obs_out, metrics_out, NULL, stream);
 * -- the same arithmetic in the same order: the two paths agree bit for bit in every run of tests/test_rollout.py and of the soak
 * loops (tests/soak_rollout.py, tests/soak_suite_context.py: profiles/r05_soak.txt), with ONE unexplained exception on record: two
 * runs of the whole GPU suite in round 4 saw a difference that never reproduced.  gym_fixed_wing.rollout.FusedRollout therefore
 * uses this call only when asked to (fused=True / "auto").  obs_io / reward_io / done_io are IN-OUT: on entry what the env's previous step (or fwg_reset, with
 * reward_io / done_io zeroed) left there, on return this step's results; the four head outputs describe the observation on
 * entry, norm_reward_out / done_prev_out the transition that led to it (each may be NULL).  Needs `head` attached to `env`
 * (fwg_attach_observer: the step phase leaves the batch moments for the NEXT head) and a configuration
 * fwg_rollout_available() accepts: a build-time / run-time specialised kernel, dense observation batch (no row log), no
 * per-env aircraft parameters; callers fall back to the two calls above otherwise.  Counts as one fwg_step and one
 * fwg_actor_act for the hipGraph rules (even numbers per captured sequence). */
int fwg_rollout_available(const fwg_handle* env, const fwg_actor* head);
int fwg_rollout_step(fwg_handle* env, fwg_actor* head, float* norm_obs_out, float* action_out, float* value_out, float* logp_out,
                     float* norm_reward_out, uint8_t* done_prev_out, float* obs_io, float* reward_io, uint8_t* done_io,
                     uint8_t* term_code_out, float* terminal_obs_out, float* metrics_out, int deterministic, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Learner side of the rollout.  fwg_gae: generalised advantage estimation over the rollout the calls above
 * filled in place -- replaces the backward loop of PPO2's runner (stable-baselines ppo2.py Runner.run) behind
 * `PPO2(policy, env).learn(...)`, reference gym_fixed_wing/examples/train_rl_controller.py:231-232.  All buffers are device
 * pointers, step-major: rewards / values / adv_out / ret_out float [n_steps][n_envs], dones uint8 [n_steps][n_envs] (the flag
 * the env returned FOR step t: the value behind it belongs to the next episode), last_value float [n_envs] (value of the
 * observation after the last step).  adv_t = delta_t + gamma lam (1 - done_t) adv_(t+1), delta_t = r_t + gamma V_(t+1)
 * (1 - done_t) - V_t; ret = adv + V.  One launch on `stream`, no synchronisation, no allocation. */
int fwg_gae(int64_t n_steps, int64_t n_envs, const float* rewards, const float* values, const uint8_t* dones,
            const float* last_value, float gamma, float lam, float* adv_out, float* ret_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * PPO update ("learner"): the minibatch step of stable-baselines' PPO2 (ppo2.py setup_model / _train_step) behind
 * `PPO2(MlpPolicy, env).learn(...)` (examples/train_rl_controller.py:223-232) on the rollout head's 64-64 networks, as HIP
 * kernels: per-minibatch advantage normalisation (biased std + 1e-8), clipped surrogate, value loss clipped around the old
 * value with the same range, entropy of the state-independent log-std, then clip_grad_norm_(max_grad_norm) (coefficient
 * max_norm / (norm + 1e-6), capped at 1) and torch.optim.Adam(eps) in torch's bias-corrected form with the step count on the
 * device.  The networks' forward and backward passes run on the matrix cores with split-bf16 operands (fwg_actor_act's
 * precision).  Parameters, Adam moments and gradients are ONE flat float32 layout, MlpPolicy.parameters() order:
 *     log_std [act_dim] | pi.0.weight [64][obs_dim], pi.0.bias [64], pi.2.weight [64][64], pi.2.bias [64],
 *     pi.4.weight [act_dim][64], pi.4.bias [act_dim] | vf.0 ... vf.4 (output width 1)
 * and for a CNN head (fwg_actor_set_conv: 5 x 12 window, 3 filters; fwg_learner_create_cnn), CnnMlpPolicy.parameters() order:
 *     log_std [act_dim] | conv.weight [5][3], conv.bias [3] | pi.1.weight [64][36], pi.1.bias [64], pi.3.weight [64][64],
 *     pi.3.bias [64], pi.5.weight [act_dim][64], pi.5.bias [act_dim] | vf.1 ... vf.5 (output width 1)
 * (13 337 floats at act_dim 3).  The conv is one module shared by both networks: tanh(conv) of the normalised window, flattened
 * feature-major, is their input, and its gradient sums both networks' terms.
 * -- fwg_learner_num_params() floats; a gradient buffer holds 4 more: the minibatch sums of the policy loss, the value loss,
 * 0.5 (logp - old logp)^2 and the clipped-ratio count.  Minibatch rows are gathered by index from the step-major rollout
 * buffers (fwg_rollout_step / fwg_actor_act outputs and fwg_gae's, flattened to [n_steps * n_envs]).  Every call takes
 * device pointers and a stream, neither synchronises nor allocates (stream-capturable), and sums in a fixed order: two
 * runs on the same inputs agree bit for bit.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fwg_learner fwg_learner;

/* Hyper-parameters, read on the DEVICE at every launch (a captured update follows changes without recapture):
 * learning rate, clip range (policy and value), entropy and value coefficients, max gradient norm, Adam betas and eps --
 * doubles, as the Python scalars torch's optimiser derives its float factors from. */
typedef struct fwg_ppo_hparams {
    double lr, cliprange, ent_coef, vf_coef, max_grad_norm, beta1, beta2, eps;
} fwg_ppo_hparams;

/* The rollout as the update reads it, rows indexed by the minibatch index arrays: obs [n][obs_dim], actions [n][act_dim],
 * values / logp (log-probability of the action at sampling time) / adv / returns [n]. */
typedef struct fwg_ppo_batch {
    const float *obs, *actions, *values, *logp, *adv, *returns;
} fwg_ppo_batch;

/* A learner for `head`'s networks (obs_dim, act_dim, device); it owns its partial-gradient scratch (~10 MB) and writes the
 * head's packed weights in fwg_actor_pack.  Destroy it before the head. */
int fwg_learner_create(fwg_actor* head, fwg_learner** out);
/* The same for a CNN head (one that fwg_actor_set_conv has given its conv): the layout includes the conv, the gradient passes
 * through it, and fwg_actor_pack writes the conv's parameters too.  fwg_learner_create refuses a CNN head and this an MLP
 * head; every other call below serves both kinds of learner.  Keep the head's kind while the learner lives. */
int fwg_learner_create_cnn(fwg_actor* head, fwg_learner** out);
void fwg_learner_destroy(fwg_learner* L);
int64_t fwg_learner_num_params(const fwg_learner* L);
/* Once per epoch: moments [n_minibatches][2] = mean and std (biased) + 1e-8 of adv over the rows
 * perm[k mb ... (k + 1) mb) (int64 row indices) of every minibatch k (ppo2.py: advs normalised per minibatch). */
int fwg_ppo_moments(fwg_learner* L, const float* adv, const int64_t* perm, int64_t mb, int n_minibatches, float* moments, void* stream);
/* The gradient half: d(pg_loss - ent_coef entropy + vf_coef vf_loss) / d params over the mb rows idx[0 .. mb) with this
 * minibatch's `moments` [2] -> grad_out [num_params + 4] (unclipped, loss sums appended).  For data-parallel training:
 * all-reduce grad_out, divide by the world size, then fwg_ppo_apply. */
int fwg_ppo_grad(fwg_learner* L, const fwg_ppo_batch* b, const int64_t* idx, int64_t mb, const float* moments, const float* params,
                 const fwg_ppo_hparams* hp, float* grad_out, void* stream);
/* The apply half: clip_grad_norm_ + Adam on params / adam_m / adam_v (each [num_params]) from `grad` ([num_params + 4]),
 * *step += 1; stats_acc [5] += pg_loss, vf_loss, entropy, approx_kl, clip_frac of the minibatch (sums / mb; entropy of the
 * log-std before the step), the order of gym_fixed_wing.ppo.STAT_KEYS. */
int fwg_ppo_apply(fwg_learner* L, const float* grad, int64_t mb, const fwg_ppo_hparams* hp, float* params, float* adam_m, float* adam_v,
                  int32_t* step, float* stats_acc, void* stream);
/* One full minibatch step: fwg_ppo_grad into the learner's own gradient buffer, then fwg_ppo_apply (three launches). */
int fwg_ppo_step(fwg_learner* L, const fwg_ppo_batch* b, const int64_t* idx, int64_t mb, const float* moments, const fwg_ppo_hparams* hp,
                 float* params, float* adam_m, float* adam_v, int32_t* step, float* stats_acc, void* stream);
/* The head's weights from the flat parameters, on the device: what fwg_actor_set_weights does from host arrays, with no host
 * round trip (a captured rollout sees the new weights at its next replay). */
int fwg_actor_pack(fwg_learner* L, const float* params, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Evaluation: the reference's evaluate_model_on_set (examples/evaluate_controller.py:44-169) without a host read per step.
 * Every scenario of a test set flies in its own env (fwg_config.auto_reset = 0) to its FIRST episode end; from then on the env
 * is fed zero actions and keeps stepping -- and keeps reporting done -- until the last scenario has ended.  Per step t:
 *     controller (fwg_pid_act, or fwg_actor_act with deterministic = 1 and frozen statistics) -> actions
 *     fwg_finish_episodes(env, metrics)      the metrics columns of the envs step t - 1 reported done
 *     fwg_eval_advance(t, ...)               folds step t - 1, zeroes the actions of finished envs
 *     fwg_step(env, actions, ..., target_out)
 * and after the last step one fwg_finish_episodes + fwg_eval_advance with actions_io = NULL.  Both calls below are stateless:
 * one launch on `stream` over caller-owned device buffers, no allocation, no synchronisation (as fwg_gae).
 * ------------------------------------------------------------------------------------------------------------------ */

/* Gains, output limits and time step of the PID baseline (pyfly.pid_controller.PIDController; the reference builds it at
 * fixed_wing.py:1281-1300 and examples/evaluate_controller.py:82-84), passed from the host BY VALUE.  Defaults of
 * gym_fixed_wing.pid.BatchedPID: k_p_phi 1, k_i_phi 0, k_d_phi 0.5 | k_p_theta -4, k_i_theta -0.75, k_d_theta -0.1 | k_p_V 0.5,
 * k_i_V 0.1 | elevator -30 .. 35 deg, aileron -30 .. 30 deg (radians here), throttle 0 .. 1 | dt 0.01. */
typedef struct fwg_pid_gains {
    float k_p_phi, k_i_phi, k_d_phi;
    float k_p_theta, k_i_theta, k_d_theta;
    float k_p_V, k_i_V;
    float delta_e_min, delta_e_max, delta_a_min, delta_a_max, delta_t_min, delta_t_max;
    float dt;
    float pad_;
} fwg_pid_gains;

/* PIDController.get_action for n_envs aircraft (examples/evaluate_controller.py:120-124,143-150).
 *   obs              : float32 [N][obs_stride], a dense observation batch (or one plane of the row log, obs_stride = n_obs)
 *   obs_cols_host    : 6 column indices into a row: roll, pitch, Va, omega_p, omega_q, omega_r (each < obs_stride)
 *   target           : float32 [N][target_stride], what fwg_step writes through target_out (info["target"])
 *   target_cols_host : 3 column indices into a row: roll, pitch, Va (each < target_stride)
 *   integrators      : float32 [3][N] IN-OUT, rows roll, pitch, Va; zero them to reset the controller
 *   actions_out      : float32 [N][3] elevator, aileron, throttle, clipped to the limits
 * aileron = -k_p_phi e_phi - k_i_phi I_phi - k_d_phi p, elevator = -k_p_theta e_theta - k_i_theta I_theta - k_d_theta (q cos phi
 * - r sin phi), throttle = -k_p_V e_Va - k_i_V I_Va with e = state - target: computed from the integrals as they stand, THEN
 * I += dt e.  A NaN input gives a NaN action (the limits do not hide it). */
int fwg_pid_act(int64_t n_envs, const float* obs, int obs_stride, const int32_t* obs_cols_host, const float* target, int target_stride,
                const int32_t* target_cols_host, fwg_pid_gains gains, float* integrators, float* actions_out, void* stream);

/* The episode tracker: call it once per step t = 0, 1, ... after the controller and before fwg_step, with the reward_out /
 * done_out / term_code_out of step t - 1 and the metrics block fwg_finish_episodes has just written (all four may be NULL at
 * t == 0, where nothing is folded).  IN-OUT, initialised by the caller before t = 0:
 *   active        : uint8 [N]   1 while the scenario's first episode is running
 *   length        : int32 [N]   steps of that episode so far
 *   termination   : uint8 [N]   FWG_TERM_* of the FIRST episode end (FWG_TERM_NONE while running)
 *   metrics_final : float32 [FWG_N_METRICS][N]  the metrics column of the FIRST episode end (untouched while running)
 *   reward_trace  : NULL or float32 [trace_steps][N]; row t - 1 is written for EVERY env: the reward where the env was active
 *                   during step t - 1, NaN where it was not -- every cell exactly once, so the buffer needs no initialisation
 *   actions_io    : NULL or float32 [N][3]; the rows of inactive envs are overwritten with zeros (stored, not multiplied: a NaN
 *                   from the policy of a finished, tumbling aircraft never reaches the step)
 * Per active env: trace[t - 1] = reward, length = t, and where done: termination = term_code, metrics_final[:] = metrics[:],
 * active = 0.  A done an env reports AFTER its first end changes nothing.  The gate sees the `active` this call leaves.
 * The last call (after the final step) passes actions_io = NULL.  Refused (FWG_ERR_INVALID): t < 0, t > trace_steps with a
 * trace, n_envs <= 0, null buffers. */
int fwg_eval_advance(int64_t n_envs, int64_t t, const float* reward, const uint8_t* done, const uint8_t* term_code, const float* metrics,
                     uint8_t* active, int32_t* length, uint8_t* termination, float* metrics_final, float* reward_trace, int64_t trace_steps,
                     float* actions_io, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Flight recorder: the episode history of up to 64 envs of a handle, kept on the device by one small launch behind every
 * fwg_reset / fwg_step -- what the reference's FixedWingAircraft keeps on the host for render / save_history
 * (fixed_wing.py:572-672) and its training callback plots every few minutes (examples/train_rl_controller.py:31-110).  Both
 * calls are stateless launches on `stream` over caller-owned device buffers: no allocation, no synchronisation, no host read,
 * and nothing passed by value changes between steps, so they may sit inside a captured sequence of fwg_step calls (one more
 * node in sequence) and replay correctly.  Buffers, for n_tracked = K envs and max_rows rows (zero `hdr` before the
 * first call: an all-zero header is "never started"):
 *   ids  : int64 [K]                        env indices of this handle; an index outside [0, N) records nothing and sets
 *                                           FWG_REC_INVALID in its slot.  An index may be listed twice (two independent slots)
 *   rows : float32 [2][K][max_rows][32]     two slabs per tracked env: the episode in progress and the last completed one
 *   hdr  : int32 [K][8]                     0: flags  FWG_REC_SLAB (bit 0: index of the OPEN slab) | FWG_REC_OPEN (an episode is
 *                                              open) | FWG_REC_OVERFLOW (the open episode lost rows) | FWG_REC_OVERFLOW_DONE (the
 *                                              completed episode did) | FWG_REC_INVALID
 *                                           1: rows in the open slab          2: rows in the completed slab
 *                                           3: FWG_TERM_* of the completed episode
 *                                           4: episode serial of the open slab (the arena's episode word, layout.cold + 3)
 *                                           5: episode serial of the completed slab
 *                                           6: episodes completed since hdr was zeroed      7: 0
 * Row (32 words, 128 B):
 *   0..15   arena sim words 0..15: e0 e1 e2 e3 p q r pn pe pd u v w elevon_r elevon_l throttle
 *   16..21  roll pitch yaw Va alpha beta: copied from layout.derived with store_derived; without it roll / pitch / yaw are
 *           computed from the committed quaternion, and Va / alpha / beta are computed from the committed state and the steady wind
 *           (turbulence off) or copied from the second derived group, which the step keeps whenever turbulence is on
 *   22..24  targets 0..2 (layout.gym + 0..2)
 *   25..27  the raw action of the step       28  its reward
 *   29      the steps_count | steps_for_target << 16 word of the arena, as bits
 *   30      done | term_code << 8, as bits   31  0
 * Row 0 of an episode is the state and target at reset (words 25..28 NaN, word 30 zero); row t >= 1 the sample after step t.
 * THE TERMINAL ROW (the one difference from the single-env class): words 25..31 are always written, but the state and target
 * words 0..24 are written only when the handle's auto_reset is off and the episode ended with FWG_TERM_STEPS or
 * FWG_TERM_SUCCESS; otherwise they are NaN.  With auto_reset on, the arena holds the NEXT episode by the time fwg_step
 * returns, so the terminal state exists nowhere (and word 29 is the next episode's); after a simulator failure the state was
 * never committed, and the single-env class records none either (fixed_wing.py:409-416).
 * A row past max_rows is dropped and FWG_REC_OVERFLOW set; nothing is ever written past a slab.
 * ------------------------------------------------------------------------------------------------------------------ */
enum { FWG_REC_SLAB = 1, FWG_REC_OPEN = 2, FWG_REC_OVERFLOW = 4, FWG_REC_OVERFLOW_DONE = 8, FWG_REC_INVALID = 16 };
int64_t fwg_record_row_words(void);            /* 32 */
/* After fwg_reset, with the same mask (NULL = all): every selected tracked env drops the episode in progress WITHOUT completing
 * it, opens its open slab again and writes row 0 from the arena.  Unselected envs' slabs and headers are left untouched. */
int fwg_record_start(const fwg_handle* h, const int64_t* ids_dev, int n_tracked, const uint8_t* mask,
                     float* rows, int32_t* hdr, int64_t max_rows, void* stream);
/* After every fwg_step, with the action batch that step consumed and its reward_out / done_out / term_code_out.  Per tracked env
 * with an open episode: appends a row; where done, closes the episode (length, termination and serial into the header, completed
 * count + 1), flips the slabs (no copy) and, with auto_reset on, opens the other slab with row 0 from the arena (the new
 * episode's reset state and target).  With auto_reset off the episode stays closed until the next fwg_record_start: a finished
 * env keeps reporting done and only the first end counts.
 * Both: FWG_ERR_INVALID for NULL buffers, n_tracked outside 1 .. 64, max_rows < 2. */
int fwg_record(const fwg_handle* h, const int64_t* ids_dev, int n_tracked, const float* actions, const float* reward,
               const uint8_t* done, const uint8_t* term_code, float* rows, int32_t* hdr, int64_t max_rows, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Training monitor (ABI 26): the undiscounted return and the length of every episode that ends during a rollout -- the `r`
 * and `l` that stable-baselines' Monitor wrapper attaches to an episode's last info and PPO2 logs as ep_rewmean / eplenmean
 * (the first job of the reference's training callback, examples/train_rl_controller.py monitor_training).  The raw reward of
 * step t is written by fwg_step itself when the caller passes row t of a [T][N] buffer as reward_out; fwg_monitor_fold folds
 * that buffer and the rollout's done flags once per rollout.  Both calls are stateless like fwg_gae: caller-owned device
 * buffers, one launch on `stream`, no allocation, no synchronisation.
 *   raw_rewards : float32 [T][N]       dones : uint8 [T][N]       (step-major, as the rollout stores them)
 *   ep_q_io     : int64 [N]            the open episode's return in units of 2^-20, carried from fold to fold (zero to start)
 *   ep_len_io   : int32 [N]            its length so far; bit 31: it holds a bad reward
 *   scratch     : fwg_monitor_scratch_bytes(N) bytes = [ceil(N / 64)][8] int64, ZEROED before the first fold (all-zero is the
 *                 identity); one slot per workgroup, updated with plain loads and stores, so folds and takes on one scratch
 *                 must be ordered (one stream)
 * Per env, in step order:
 *   q_t = (int64) rintf(r_t * 1048576.f)          (the product is exact in float; ties round to even)
 *   r_t is BAD when !(fabsf(r_t) <= 1048576.f)    (NaN, inf, out of the bound)
 *   good: ep_q += q_t;  bad: bit 31 of ep_len is set;  both: ep_len += 1
 *   dones[t][e] != 0: the episode is emitted WITH the reward of step t, then (ep_q, ep_len) = (0, 0).  A flagged episode adds 1
 *   to `nonfinite` and nothing else; any other updates episodes, sum_q, sum_len, min_q, max_q, min_len, max_len.
 * Bounds: |r_t| <= 2^20 and steps_max < 65 535, so |ep_q| < 2^56.  All sums are integers: the result is independent of the
 * kernel's split over time, of wave order and of how envs are sharded over ranks (bit for bit); the quantisation costs at most
 * 2^-21 per step.  Several folds before one take accumulate.
 * fwg_monitor_take writes FWG_N_MONITOR doubles to `out` (device): 0 episodes, 1 nonfinite, 2 sum_return = sum_q / 2^20,
 * 3 sum_length, 4 min_return, 5 max_return, 6 min_length, 7 max_length (with no episode the minima are +inf and the maxima
 * -inf), and resets the scratch to the identity.
 * Both: FWG_ERR_INVALID for a NULL buffer, n_steps < 1, n_envs < 1 (nothing is launched).
 * ------------------------------------------------------------------------------------------------------------------ */
int64_t fwg_monitor_scratch_bytes(int64_t n_envs);   /* 0 for n_envs < 1 */
int fwg_monitor_fold(int64_t n_steps, int64_t n_envs, const float* raw_rewards, const uint8_t* dones, int64_t* ep_q_io,
                     int32_t* ep_len_io, void* scratch, void* stream);
int fwg_monitor_take(int64_t n_envs, void* scratch, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Goal env: the reference's FixedWingAircraftGoal (a gym.GoalEnv, fixed_wing.py:1165-1277) for a whole batch -- the goal views of
 * a dict observation, compute_reward(achieved_goal, desired_goal, info) for substituted goals, and hindsight relabelling ("future"
 * strategy) of one rollout.  The exports are additions to ABI 26: no struct or call that existed changes.  All launches are
 * stateless: caller-owned device buffers, the caller's stream, no allocation, no synchronisation, no atomics, and nothing passed by
 * value changes from step to step, so they may sit inside a captured sequence of fwg_step calls.
 *
 * GOAL ROWS are float32 [..][4] (16 bytes): words 0..2 the scaled goals (x - mean) / var in the spec's order, unused words 0;
 * word 3 per buffer, below.
 *
 * fwg_goal_spec, a host struct passed by pointer: which target states are goals and how they are scaled.  A goal must be one of the
 * handle's target states (its slot k in target.states) and one of roll / pitch / Va.  The reward description is NOT part of it:
 * the kernels read the handle's lowered configuration in device memory, so fwg_update_config is seen by the next launch.
 * step_count_mode selects the step counter the action-delta factor sees: 0 = compute_reward's (steps_count = info["step"]: the
 * factor is off for transitions 0 and 1, the reference's behaviour), 1 = step()'s (off for transition 0 only: with the goals a
 * transition really had the result is the reward the step gave).
 *
 * THE REWARD FUNCTION (both fwg_goal_reward and fwg_goal_relabel) is get_reward (fixed_wing.py:674-774) with success = False for
 * the unscaled achieved goals as state values and the unscaled desired goals as targets: wrapped errors as in the step; function
 * classes linear (with max), quadratic, exponential; forms absolute and potential (previous shaping values from `prev` with the
 * action before, and -- the reference's quirk -- the same action list for its value and delta factors); action factors from the
 * window of raw actions; goal-class factors from the substituted errors and the configured bounds; success-class factors 0; the
 * step class its constant.  Refused with FWG_ERR_INVALID and a message naming the factor -- what cannot be defined from a
 * transition alone: int_error factors, reward.randomize_scaling, a state / error / goal factor that names a state or a bounded
 * target that is not a goal, a shaping action-bound factor under the potential form without a delta factor's window; and, for
 * fwg_goal_relabel only, linear / sinusoidal targets, resample_every > 0, on_success == "new" (the goal must be constant within an
 * episode).  A refusal launches nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fwg_goal_spec {
    int32_t n_goals;           /* 1 .. 3 */
    int32_t step_count_mode;   /* 0: compute_reward's counter, 1: step()'s */
    int32_t k[3];              /* per goal: index into target.states */
    int32_t pad_;
    float mean[3], var[3];     /* observation.goals[i]: scaled = (x - mean) / var (the kernels divide, as the reference does) */
    float inv_var[3];          /* 1 / var, for callers that scale on their own; the kernels do not read it */
    float pad2_;
} fwg_goal_spec;
enum { FWG_GOAL_KEPT = -1, FWG_GOAL_TERMINAL = -2, FWG_GOAL_NO_WINDOW = -3 };   /* src_row_out values below 0 */
/* W: the largest window_size of the configuration's action-delta factors, 1 when there is none (host function). */
int fwg_goal_window(const fwg_handle* h);
/* One lane per env.  achieved [N][4]: the goal states of the committed state -- bit-equal to (w - mean) / var of the flight
 * recorder's words 16 / 17 / 19 -- and in word 3 the arena's step word (layout.gym + 3) as raw bits: its low 16 bits are the
 * episode's transition count so far.  desired [N][4]: the current targets (layout.gym + 0..2), word 3 = 0.  After a done step under
 * auto_reset both show the new episode (count 0). */
int fwg_goal_observe(const fwg_handle* h, const fwg_goal_spec* spec, float* achieved, float* desired, void* stream);
/* The batched compute_reward: one lane per transition, m transitions.
 *   achieved, desired : [m][4] goal rows after the transition / the goals to evaluate against
 *   prev              : [m][4] goal rows before the transition; may be NULL unless the reward form is potential
 *   act_win           : [W][m][4] raw actions (a0 a1 a2 -), W = fwg_goal_window: row W - 1 the transition's own action, row W - 1 - j
 *                       the one j steps before it in the same episode; rows older than step[i] actions back are never read as values
 *   step              : int32 [m] index of the transition in its episode        reward_out : float32 [m] */
int fwg_goal_reward(const fwg_handle* h, const fwg_goal_spec* spec, int64_t m, const float* achieved, const float* desired,
                    const float* prev, const float* act_win, const int32_t* step, float* reward_out, void* stream);
/* HER's "future" strategy over one rollout of the handle's N envs, step-major as FusedRollout keeps it:
 *   achieved, desired : [T + 1][N][4] rows of fwg_goal_observe: row 0 before step 0, row t + 1 behind step t
 *   actions [T][N][3], raw_rewards [T][N], dones uint8 [T][N]
 *   desired_out [T][N][4], reward_out [T][N], src_row_out int32 [T][N]
 * For transition (t, n), idx = low 16 bits of word 3 of achieved[t][n], W = fwg_goal_window:
 *   dones[t][n]: src = -2 (under auto-reset the achieved goal after a terminal step is not in the buffer);
 *   else, if the configuration has a delta factor and min(idx, W - 1) > t: src = -3 (the window reaches before row 0);
 *   else R = the first t_e > t with dones[t_e][n], or T; b = philox4x32(env_id_base + n, serial, t, 10, seed_lo, seed_hi);
 *        (uint64) b.y >= p_scaled: src = -1; otherwise src = r = t + 1 + (uint32)(((uint64) b.x * (uint64)(R - t)) >> 32), the new
 *        goal is words 0..2 of achieved[r][n], reward_out = the reward function on achieved[t + 1][n], the new goal, prev =
 *        achieved[t][n], the window actions[t - j][n], step = idx; desired_out = the new goal with word 3 = 0.
 *   wherever src < 0: desired_out = desired[t][n] (word 3 = 0) and reward_out = raw_rewards[t][n], bit for bit.
 * p_scaled in [0, 2^32]: 2^32 relabels every eligible transition.  Sharding envs over handles with their env_id_base gives the
 * columns of the whole, bit for bit. */
int fwg_goal_relabel(const fwg_handle* h, const fwg_goal_spec* spec, int64_t n_steps, const float* achieved, const float* desired,
                     const float* actions, const float* raw_rewards, const uint8_t* dones, uint64_t seed, uint32_t serial,
                     uint64_t p_scaled, float* desired_out, float* reward_out, int32_t* src_row_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Hindsight replay: what an off-policy learner puts between a goal env and its update -- many rollouts kept on the device
 * ("slots"), minibatches drawn uniformly over all of them, and a fresh hindsight goal with that goal's reward every time a
 * transition is drawn (fwg_goal_relabel relabels one rollout once, in place).  The exports are additions to ABI 26: no struct or
 * call that existed changes.  Both launches are stateless: caller-owned device buffers, the caller's stream, no allocation, no
 * synchronisation, no atomics.  A refusal launches nothing and returns FWG_ERR_INVALID with a message.
 *
 * fwg_replay_index, once per stored rollout (it needs no handle): dones uint8 [T][N] -> ep_end int32 [T][N],
 *   ep_end[t][n] = the first t_e > t with dones[t_e][n], or T when there is none (the R of fwg_goal_relabel).
 * Refused: a NULL buffer, n_steps outside 1 .. 2^31 - 2, n_envs < 1.
 *
 * fwg_replay_view, a host struct passed by pointer: the slots.  Slot-major device buffers, K = n_slots of them allocated and the
 * first n_filled holding rollouts of the handle's N envs over T steps:
 *   obs [K][T + 1][N][D] (row t the observation before step t, row T the one behind the last step; D = obs_words, 1 .. 240)
 *   actions [K][T][N][3], raw_rewards [K][T][N], dones uint8 [K][T][N], ep_end int32 [K][T][N] (fwg_replay_index per slot)
 *   achieved, desired [K][T + 1][N][4]: the goal rows of fwg_goal_observe -- row 0 before step 0, row t + 1 behind step t, the step
 *   word in word 3 of achieved.
 *
 * fwg_replay_sample draws `batch` transitions (1 .. 2^32 - 1).  With mulhi(x, m) = (uint32)(((uint64) x * m) >> 32), sample i is:
 *   a = philox4x32(i, serial, 0, 11, seed_lo, seed_hi); slot k = mulhi(a.x, n_filled), t = mulhi(a.y, T), n = mulhi(a.z, N)
 *       (uniform over the stored transitions, with replacement);
 *   idx = low 16 bits of word 3 of achieved[k][t][n], W = fwg_goal_window, R = ep_end[k][t][n];
 *   dones[k][t][n]: src = -2;
 *   else, if the configuration has a delta factor and min(idx, W - 1) > t: src = -3 (the window reaches before row 0);
 *   else, if (uint64) a.w >= p_scaled: src = -1;
 *   else src = a row r of the same slot and episode, with b = philox4x32(i, serial, 1, 11, seed_lo, seed_hi):
 *       FWG_REPLAY_FUTURE   r = t + 1 + mulhi(b.x, R - t)                      (a row behind the transition: t < r <= R)
 *       FWG_REPLAY_FINAL    r = R                                              (the last row of the episode the slot holds)
 *       FWG_REPLAY_EPISODE  s0 = max(t - idx, 0), r = s0 + 1 + mulhi(b.x, R - s0)   (any row of the episode: s0 < r <= R)
 *     the goal never comes from outside the slot, nor from across a done;
 *   src >= 0: the new goal is words 0..2 of achieved[k][r][n]; reward_out = the reward function (above, under
 *       spec->step_count_mode) on achieved[k][t + 1][n], the new goal, prev = achieved[k][t][n], the window actions[k][t - j][n],
 *       step = idx;
 *   src < 0: the goal is desired[k][t][n] and reward_out = raw_rewards[k][t][n], bit for bit.
 * Outputs, one row per sample: obs_out [B][D] = obs[k][t][n], next_obs_out [B][D] = obs[k][t + 1][n], action_out [B][3],
 * achieved_out [B][4] = achieved[k][t + 1][n] and desired_out [B][4] the goal (word 3 = 0 in both), reward_out [B], done_out uint8
 * [B] = dones[k][t][n], index_out int32 [B][4] = (k, t, n, src).
 * UNDER AUTO-RESET the rows behind a terminal step show the NEXT episode: next_obs_out and achieved_out of a sample with done_out
 * set are the first observation and goals of the episode that follows (the learner masks the bootstrap with done_out).
 * Refused: what fwg_goal_relabel refuses (the configuration, NULL buffers, n_steps, p_scaled > 2^32), and a view of another N than
 * the handle's, n_filled < 1 or > n_slots, an unknown strategy, obs_words outside 1 .. 240, batch outside 1 .. 2^32 - 1.
 * ------------------------------------------------------------------------------------------------------------------ */
#define FWG_REPLAY_MAX_OBS 240
enum { FWG_REPLAY_FUTURE = 0, FWG_REPLAY_FINAL = 1, FWG_REPLAY_EPISODE = 2 };
typedef struct fwg_replay_view {
    int64_t n_slots, n_filled;   /* K allocated, 1 .. K of them hold a rollout */
    int64_t n_steps, n_envs;     /* T; N, the handle's */
    int32_t obs_words, pad_;     /* D */
    const float* obs;
    const float* actions;
    const float* raw_rewards;
    const uint8_t* dones;
    const int32_t* ep_end;
    const float* achieved;
    const float* desired;
} fwg_replay_view;
int fwg_replay_index(int64_t n_steps, int64_t n_envs, const uint8_t* dones, int32_t* ep_end, void* stream);
int fwg_replay_sample(const fwg_handle* h, const fwg_goal_spec* spec, const fwg_replay_view* view, int strategy, int64_t batch,
                      uint64_t seed, uint32_t serial, uint64_t p_scaled, float* obs_out, float* next_obs_out, float* action_out,
                      float* achieved_out, float* desired_out, float* reward_out, uint8_t* done_out, int32_t* index_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Off-policy update: what learns from the minibatches of fwg_replay_sample -- DDPG, or with two critics and a policy delay TD3's
 * clipped double-Q and delayed actor step, as HIP kernels on the scheme of the PPO update (64-row tiles in LDS, bf16 matrix cores
 * with every fp32 operand split hi + lo, one partial-gradient slab per workgroup summed in a fixed order: no float atomics, the
 * update is bitwise deterministic run to run).  The exports are additions to ABI 26: no struct or call that existed changes.
 *
 * Sizes: D = obs_words, G = goal_words (1 .. 4), A = act_dim (1 .. 4); the actor reads [o | g] (D + G words), a critic [o | g | a]
 * (D + G + A words), and D + G + A <= 64 (one 64-wide LDS tile holds a row).  Hidden layers 64-64 with ReLU:
 *   pi(o, g)     = tanh(W3 relu(W2 relu(W1 [o | g] + b1) + b2) + b3)
 *   Q_j(o, g, a) = w3 relu(W2 relu(W1 [o | g | a] + b1) + b2) + b3,   j < n_critics (1: DDPG, 2: TD3's twin critics)
 * Online and target parameters are two flat float32 vectors with one layout, torch's parameters() order of
 * nn.Sequential(Linear, ReLU, Linear, ReLU, Linear[, Tanh]):  actor | critic 0 | critic 1, each
 *   W1 [64][K]  b1 [64]  W2 [64][64]  b2 [64]  W3 [nout][64]  b3 [nout]
 * -- fwg_offpolicy_num_params() floats, the first fwg_offpolicy_actor_params() of them the actor's ("segment" FWG_DDPG_ACTOR; the
 * rest is segment FWG_DDPG_CRITICS).  Adam's moments have the same layout.  A gradient buffer holds 4 more floats behind it, batch
 * sums: sum_j sum (Q_j(o,g,a) - y)^2, sum Q_0(o,g,pi(o,g)), sum Q_0(o,g,a), sum y.
 *
 * Update u (counting from 1) on B rows (o, o', a, g, r, done):
 *   critic step: a' = pi_target(o', g), q' = min_j Q_target,j(o', g, a'), y = r + gamma (1 - done) q' (no gradient through y; y is r
 *     itself, bit for bit, on a row with done set and at gamma = 0), L_c = sum_j mean_B (Q_j(o,g,a) - y)^2, Adam on the critics;
 *   if u % policy_delay == 0, the actor step with the critics as just updated: L_a = -mean_B Q_0(o, g, pi(o,g)), Adam on the actor
 *     (the critics' gradient words are neither computed nor written), then theta_target <- lerp(theta_target, theta, tau) on everything.
 * Adam is torch.optim.Adam's form; the bias corrections are computed from doubles.  max_grad_norm_* > 0 clips first, PER SEGMENT
 * (clip_grad_norm_ over the segment's words): the actor's gradient by its own norm, the critics' by one joint norm over both
 * critics -- they are one optimiser's parameters; <= 0: no clipping.  TD3's target-policy smoothing noise is not part of it.
 *
 * fwg_offpolicy_batch, device pointers: obs, next_obs [B][D], action [B][A], goal_rows [B][4] (row stride 4 words whatever G is:
 * fwg_replay_sample's desired_out as it stands), reward [B], done uint8 [B].  fwg_ddpg_hparams is a HOST struct, read at the call.
 * All launches go to the caller's stream; nothing synchronises or allocates after fwg_offpolicy_create (which allocates on the
 * current device; it takes no env handle and no head).  A learner owns ONE set of partial-gradient slabs and one gradient buffer,
 * which both gradient calls and fwg_ddpg_step reuse: it serves one stream at a time -- calls on one learner from two streams must be
 * ordered by the caller (a learner per stream otherwise).
 * Refused with FWG_ERR_INVALID and a message naming the argument (nothing is launched): a NULL pointer, B < 1, goal_words or act_dim
 * outside 1 .. 4, n_critics outside {1, 2}, D + G + A > 64 (the message gives the three sizes), a segment other than 0 / 1,
 * update < 1, policy_delay < 1.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct fwg_offpolicy fwg_offpolicy;
enum { FWG_DDPG_ACTOR = 0, FWG_DDPG_CRITICS = 1 };
typedef struct fwg_offpolicy_batch {
    const float* obs;
    const float* next_obs;
    const float* action;
    const float* goal_rows;
    const float* reward;
    const uint8_t* done;
} fwg_offpolicy_batch;
typedef struct fwg_ddpg_hparams {
    double gamma, tau, lr_actor, lr_critic, beta1, beta2, eps, max_grad_norm_actor, max_grad_norm_critic;
} fwg_ddpg_hparams;
int fwg_offpolicy_create(int obs_words, int goal_words, int act_dim, int n_critics, fwg_offpolicy** out);
void fwg_offpolicy_destroy(fwg_offpolicy* learner);
int64_t fwg_offpolicy_num_params(const fwg_offpolicy* learner);
int64_t fwg_offpolicy_actor_params(const fwg_offpolicy* learner);
/* The critics' segment of grad_out [P + 4] and the loss sums 0, 2, 3 (two launches: the gradient slabs, their reduction); the
 * actor's segment and sum 1 are left as they are.  td_target_out: NULL, or [B] receives y. */
int fwg_ddpg_critic_grad(fwg_offpolicy* learner, const fwg_offpolicy_batch* batch, int64_t B, const fwg_ddpg_hparams* hparams, const float* params,
                         const float* target_params, float* grad_out, float* td_target_out, void* stream);
/* The actor's segment of grad_out and loss sum 1; the critics' segment and sums 0, 2, 3 are left as they are. */
int fwg_ddpg_actor_grad(fwg_offpolicy* learner, const fwg_offpolicy_batch* batch, int64_t B, const float* params, float* grad_out, void* stream);
/* Adam on one segment of params / adam_m / adam_v with steps[segment] (int32 [2], on the device) as its step counter; stats_acc [4]
 * (critic_loss, actor_loss, q_mean, target_mean) += that segment's statistics of the batch (critics: 0, 2, 3; actor: 1).  The other
 * segment, its moments and its counter are not touched.  target_params: NULL, or the Polyak pass over the WHOLE vector follows. */
int fwg_ddpg_apply(fwg_offpolicy* learner, int segment, const float* grad, int64_t B, const fwg_ddpg_hparams* hparams, float* params, float* adam_m,
                   float* adam_v, int32_t* steps, float* stats_acc, float* target_params, void* stream);
/* One whole update `update` (>= 1) into the learner's own gradient buffer: the critic step (three launches), and when
 * update % policy_delay == 0 -- decided here, on the host -- the actor step and the Polyak pass (four more). */
int fwg_ddpg_step(fwg_offpolicy* learner, const fwg_offpolicy_batch* batch, int64_t B, int64_t update, int policy_delay, const fwg_ddpg_hparams* hparams,
                  float* params, float* target_params, float* adam_m, float* adam_v, int32_t* steps, float* stats_acc, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Behaviour head: the behaviour policy of an off-policy learner between two env steps of an exploration rollout, as ONE launch
 * (one workgroup per 64 envs).  An addition to ABI 26: no struct or call that existed changes.
 *
 * Sizes as in "Off-policy update": D observation words, G goal words (1 .. 4), A actions (1 .. 4), D + G + A <= 64.  params: device
 * pointer to the actor's parameters, flat fp32 in the actor's layout there (W1 [64][D + G] b1 W2 b2 W3 [A][64] b3) -- the first
 * fwg_offpolicy_actor_params words of a learner's online vector, read in place at every launch.
 *
 * Per env e < N, in this order:
 *   goal rows    env given: achieved_out[e] / desired_out[e] ([N][4]) = what fwg_goal_observe writes for the env's state, bit for
 *                bit; the actor's goal is desired_out[e][0 .. G).  No env: goal_rows[e][0 .. G) as given ([N][4]).
 *   obs_out      NULL, or [N][D] receives obs[e] (the rollout's observation row: no copy launch)
 *   pi           tanh(actor([obs[e] | goal]))
 *   exploration  unless `deterministic`: c = draws[e] (uint32 [N], device), draws[e] = c + 1 -- no counter travels by value, so a
 *                captured launch replays correctly.  Philox blocks philox4x32(env_id_base + e, c, sub, 12, seed lo, seed hi) (12:
 *                the stream of these draws): sub 0 -> normals n_0 .. n_3 by Box-Muller; sub 1 -> uniforms u_i = 2 u01(x_i) - 1;
 *                sub 2, word 0 < eps_scaled -> the action is (u_0 .. u_{A-1}), else clamp(pi_i + sigma n_i, -1, 1).
 *                noise_params (uint32 [4], device): sigma as float bits, eps_scaled = min(2^32, round(eps 2^32)) as low word and
 *                high word, 0.  `deterministic` neither reads nor writes draws or noise_params.
 *   stores       action_out[e][0 .. A); done_out[e] = done_in[e] when both are given (uint8 [N]; both or neither).
 * The launch goes to `stream`; nothing synchronises or allocates.
 * Refused with FWG_ERR_INVALID and a message naming the argument (nothing is launched): D + G > 64, D + G + A > 64 (the message
 * gives the three sizes), G or A outside 1 .. 4, both or neither of env / goal_rows, an env that writes a row log (obs_log_rows
 * != 0), N / D / G that are not the env's, a NULL required pointer (params, obs, action_out, draws, noise_params; with an env
 * goal_spec, achieved_out, desired_out), N < 1.
 * ------------------------------------------------------------------------------------------------------------------ */
int fwg_behaviour_act(const fwg_handle* env, const fwg_goal_spec* goal_spec, int64_t N, int D, int G, int A, const float* params, const float* obs,
                      const float* goal_rows, float* achieved_out, float* desired_out, float* obs_out, float* action_out, const uint8_t* done_in,
                      uint8_t* done_out, uint32_t* draws, const uint32_t* noise_params, uint64_t seed, uint32_t env_id_base, int deterministic,
                      void* stream);

/* Global step counter driving the ring slots (diagnostics/tests). */
int64_t fwg_global_step(const fwg_handle* h);

const char* fwg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FWGYM_H */
