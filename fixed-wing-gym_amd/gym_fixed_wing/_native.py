"""ctypes binding of libfwgym.so (include/fwgym.h).  The HIP library is the ONLY compute backend: importing this
module without a built library raises, there is no CPU fallback."""
import ctypes as C
import os

FWG_ABI_VERSION = 26
N_VARS = 23
N_RESET_VARS = 21
N_PARAMS = 49
MAX_OBS = 32
MAX_ROWS = 8
MAX_FACTORS = 16
MAX_TARGETS = 3
MAX_WINDOW = 8
MAX_STREAK = 128
END_WINDOW = 50
N_DRYDEN = 8
N_METRICS = 28
N_REDUCE = 16
N_MONITOR = 8

VARS = ["roll", "pitch", "yaw", "omega_p", "omega_q", "omega_r", "position_n", "position_e", "position_d",
        "velocity_u", "velocity_v", "velocity_w", "Va", "alpha", "beta", "elevator", "aileron", "throttle",
        "wind_n", "wind_e", "wind_d", "elevon_right", "elevon_left"]
VAR_ID = {n: i for i, n in enumerate(VARS)}
PARAMS = ["mass", "Jx", "Jy", "Jz", "Jxz", "S_wing", "b", "c", "S_prop", "C_prop", "k_motor", "k_T_P", "k_Omega",
          "e", "ar", "M", "a_0", "C_L_0", "C_L_alpha", "C_L_q", "C_L_delta_e", "C_D_p", "C_D_beta1", "C_D_beta2",
          "C_D_q", "C_D_delta_e", "C_m_0", "C_m_alpha", "C_m_q", "C_m_delta_e", "C_m_fp", "C_Y_0", "C_Y_beta",
          "C_Y_p", "C_Y_r", "C_Y_delta_a", "C_Y_delta_r", "C_l_0", "C_l_beta", "C_l_p", "C_l_r", "C_l_delta_a",
          "C_l_delta_r", "C_n_0", "C_n_beta", "C_n_p", "C_n_r", "C_n_delta_a", "C_n_delta_r"]
assert len(PARAMS) == N_PARAMS and len(VARS) == N_VARS

TERM_NONE, TERM_STEPS, TERM_SUCCESS, TERM_VAR0, TERM_NAN = 0, 1, 2, 16, 255
OBS_STATE, OBS_TARGET_RELATIVE, OBS_TARGET_ABSOLUTE, OBS_ACTION, OBS_TARGET_INTEGRATOR = 0, 1, 2, 3, 4
TGT_CONSTANT, TGT_COMPENSATE, TGT_LINEAR, TGT_SINUSOIDAL = 0, 1, 2, 3
RC_STATE, RC_ACTION, RC_SUCCESS, RC_STEP, RC_GOAL = 0, 1, 2, 3, 4
RT_VALUE, RT_ERROR, RT_DELTA, RT_BOUND, RT_PER_STATE, RT_ALL, RT_INT_ERROR = 0, 1, 2, 3, 4, 5, 6
FC_LINEAR, FC_QUADRATIC, FC_EXPONENTIAL = 0, 1, 2
ON_SUCCESS = {"none": 0, "done": 1, "new": 2}
TURB_FILTER, TURB_INCREMENT = 0, 1

# rows of the metrics block
M_RISE_TIME, M_SETTLING_TIME, M_OVERSHOOT, M_TOTAL_ERROR, M_AVG_ERROR = 0, 3, 7, 10, 13
M_CONTROL_VARIATION, M_SUCCESS, M_SUCCESS_TIME_FRAC, M_END_ERROR = 16, 17, 21, 25


def term_name(code):
    """info["termination"] string of a termination code (reference fixed_wing.py:368,385,416)."""
    code = int(code)
    if code == TERM_STEPS:
        return "steps"
    if code == TERM_SUCCESS:
        return "success"
    if code == TERM_NAN:
        return "nan"
    if TERM_VAR0 <= code < TERM_VAR0 + N_VARS:
        return VARS[code - TERM_VAR0]
    return None


class ObsDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("src", C.c_int32), ("window", C.c_int32), ("norm", C.c_int32),
                ("mean", C.c_double), ("var", C.c_double)]


class TargetDesc(C.Structure):
    _fields_ = [("var", C.c_int32), ("cls", C.c_int32), ("wrap", C.c_int32), ("has_delta", C.c_int32),
                ("has_bound", C.c_int32), ("pad_", C.c_int32),
                ("low", C.c_double), ("high", C.c_double), ("delta", C.c_double), ("bound", C.c_double),
                ("slope_low", C.c_double), ("slope_high", C.c_double),
                ("amplitude_low", C.c_double), ("amplitude_high", C.c_double),
                ("period_low", C.c_double), ("period_high", C.c_double)]


class FactorDesc(C.Structure):
    _fields_ = [("cls", C.c_int32), ("type", C.c_int32), ("src", C.c_int32), ("fclass", C.c_int32),
                ("shaping", C.c_int32), ("window", C.c_int32), ("has_max", C.c_int32),
                ("value_is_timesteps", C.c_int32),
                ("sign", C.c_double), ("scaling", C.c_double), ("max", C.c_double), ("value", C.c_double)]


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("struct_bytes", C.c_uint32),
        ("dt", C.c_double), ("rho", C.c_double), ("g", C.c_double),
        ("n_substeps", C.c_int32), ("actuator_microsteps", C.c_int32), ("turbulence", C.c_int32), ("turbulence_output", C.c_int32),
        ("param", C.c_double * N_PARAMS),
        ("con_min", C.c_double * N_VARS), ("con_max", C.c_double * N_VARS),
        ("val_min", C.c_double * N_VARS), ("val_max", C.c_double * N_VARS),
        ("init_min", C.c_double * N_VARS), ("init_max", C.c_double * N_VARS),
        ("elevon_omega0", C.c_double * 2), ("elevon_zeta", C.c_double * 2), ("elevon_dot_max", C.c_double * 2),
        ("throttle_tau", C.c_double),
        ("dryden_A", C.c_double * (N_DRYDEN * N_DRYDEN)), ("dryden_B", C.c_double * (N_DRYDEN * 4)),
        ("dryden_C", C.c_double * (6 * N_DRYDEN)),
        ("steps_max", C.c_int32), ("obs_length", C.c_int32), ("obs_step", C.c_int32), ("n_obs", C.c_int32),
        ("obs_normalize", C.c_int32), ("obs_noise", C.c_int32),
        ("obs_noise_mean", C.c_double), ("obs_noise_std", C.c_double),
        ("obs", ObsDesc * MAX_OBS),
        ("n_actions", C.c_int32), ("scale_actions", C.c_int32),
        ("scale_low", C.c_double), ("scale_high", C.c_double),
        ("act_to_low", C.c_double * 3), ("act_to_high", C.c_double * 3),
        ("has_action_bounds", C.c_int32), ("pad0_", C.c_int32),
        ("act_bound_min", C.c_double * 3), ("act_bound_max", C.c_double * 3),
        ("n_targets", C.c_int32), ("resample_every", C.c_int32), ("streak_req", C.c_int32), ("on_success", C.c_int32),
        ("streak_fraction", C.c_double),
        ("target", TargetDesc * MAX_TARGETS),
        ("reward_potential", C.c_int32), ("step_fail_timesteps", C.c_int32),
        ("step_fail_value", C.c_double),
        ("term_present", C.c_int32 * 3), ("n_factors", C.c_int32),
        ("term_weight", C.c_double * 3),
        ("factor", FactorDesc * MAX_FACTORS),
        ("metrics", C.c_int32), ("auto_reset", C.c_int32), ("store_derived", C.c_int32), ("obs_log_rows", C.c_int32),
        ("rise_low", C.c_double), ("rise_high", C.c_double),
        ("model_n", C.c_int32), ("model_dist", C.c_int32), ("model_idx", C.c_int32 * N_PARAMS), ("pad_model_", C.c_int32),
        ("model_var", C.c_double * N_PARAMS), ("model_clip_lo", C.c_double * N_PARAMS), ("model_clip_hi", C.c_double * N_PARAMS),
        ("randomize_scaling", C.c_int32), ("integration_window", C.c_int32),
        ("sk_n_intensity", C.c_int32), ("sk_n_turbulence", C.c_int32), ("sk_index_intensity", C.c_int32), ("sk_index_turbulence", C.c_int32),
        ("sk_cum_intensity", C.c_double * 4), ("sk_gain_intensity", C.c_double * 4),
        ("sk_cum_turbulence", C.c_double * 2), ("sk_on_turbulence", C.c_double * 2), ("sk_base_gain", C.c_double),
        ("factor_scaling_low", C.c_double * MAX_FACTORS), ("factor_scaling_high", C.c_double * MAX_FACTORS),
    ]


class Layout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ["rows", "sim", "cold", "derived", "gym", "tprop", "goal", "act_ring", "cmd_ring", "end_ring", "lag_ring",
                 "window", "lag_depth", "lag_groups", "draw", "aero", "aero_next", "fscale", "fscale_next", "model_raw", "model_raw_next", "fin"]]


class ActorWeights(C.Structure):
    """fwg_actor_weights: float32 host arrays in torch.nn.Linear layout."""
    _fields_ = [(n, C.POINTER(C.c_float)) for n in
                ["pi_w0", "pi_b0", "pi_w1", "pi_b1", "pi_w2", "pi_b2", "vf_w0", "vf_b0", "vf_w1", "vf_b1", "vf_w2", "vf_b2",
                 "log_std"]]


class ActorStats(C.Structure):
    """fwg_actor_stats: VecNormalize's obs_rms / ret_rms."""
    _fields_ = [("obs_mean", C.c_float * 64), ("obs_var", C.c_float * 64), ("obs_count", C.c_float),
                ("ret_mean", C.c_float), ("ret_var", C.c_float), ("ret_count", C.c_float)]


class PpoHparams(C.Structure):
    """fwg_ppo_hparams: the update's hyper-parameters, read on the device at every launch."""
    _fields_ = [(n, C.c_double) for n in ["lr", "cliprange", "ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps"]]


class PpoBatch(C.Structure):
    """fwg_ppo_batch: device pointers of the flattened rollout buffers."""
    _fields_ = [(n, C.c_void_p) for n in ["obs", "actions", "values", "logp", "adv", "returns"]]


class PidGains(C.Structure):
    """fwg_pid_gains: gains, output limits (radians / throttle fraction) and time step of the PID baseline, passed by value."""
    _fields_ = [(n, C.c_float) for n in
                ["k_p_phi", "k_i_phi", "k_d_phi", "k_p_theta", "k_i_theta", "k_d_theta", "k_p_V", "k_i_V",
                 "delta_e_min", "delta_e_max", "delta_a_min", "delta_a_max", "delta_t_min", "delta_t_max", "dt", "pad_"]]


# the flight recorder's row and header (include/fwgym.h "Flight recorder")
REC_WORDS, REC_HDR, REC_MAX_TRACKED = 32, 8, 64
REC_SLAB, REC_OPEN, REC_OVERFLOW, REC_OVERFLOW_DONE, REC_INVALID = 1, 2, 4, 8, 16

class GoalSpecStruct(C.Structure):
    """fwg_goal_spec (include/fwgym.h "Goal env"): which target states are goals, their scaling, the delta factor's step counter."""
    _fields_ = [("n_goals", C.c_int32), ("step_count_mode", C.c_int32), ("k", C.c_int32 * 3), ("pad_", C.c_int32),
                ("mean", C.c_float * 3), ("var", C.c_float * 3), ("inv_var", C.c_float * 3), ("pad2_", C.c_float)]


GOAL_KEPT, GOAL_TERMINAL, GOAL_NO_WINDOW = -1, -2, -3   # fwg_goal_relabel's src_row_out values below 0
STREAM_GOAL = 10                                        # Philox stream of the relabelling draws

class ReplayView(C.Structure):
    """fwg_replay_view (include/fwgym.h "Hindsight replay"): the sizes and the slot-major device buffers of a replay buffer."""
    _fields_ = [("n_slots", C.c_int64), ("n_filled", C.c_int64), ("n_steps", C.c_int64), ("n_envs", C.c_int64),
                ("obs_words", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ["obs", "actions", "raw_rewards", "dones", "ep_end", "achieved", "desired"]]


REPLAY_STRATEGIES = {"future": 0, "final": 1, "episode": 2}   # FWG_REPLAY_FUTURE / _FINAL / _EPISODE
REPLAY_MAX_OBS = 240                                            # FWG_REPLAY_MAX_OBS
STREAM_REPLAY = 11                                              # Philox stream of the replay draws

PPO_NSTAT = 4   # loss sums appended to a gradient buffer (include/fwgym.h "PPO update")


class OffpolicyBatch(C.Structure):
    """fwg_offpolicy_batch (include/fwgym.h "Off-policy update"): device pointers of one minibatch; goal rows have a stride of 4."""
    _fields_ = [(n, C.c_void_p) for n in ["obs", "next_obs", "action", "goal_rows", "reward", "done"]]


class DdpgHparams(C.Structure):
    """fwg_ddpg_hparams: a host struct, read when a call is issued.  max_grad_norm_* <= 0: no clipping."""
    _fields_ = [(n, C.c_double) for n in ["gamma", "tau", "lr_actor", "lr_critic", "beta1", "beta2", "eps", "max_grad_norm_actor",
                                          "max_grad_norm_critic"]]


DDPG_NSTAT = 4                      # loss sums appended to a gradient buffer (include/fwgym.h "Off-policy update")
DDPG_ACTOR, DDPG_CRITICS = 0, 1     # FWG_DDPG_ACTOR / FWG_DDPG_CRITICS: the two segments of the flat parameter vector
STREAM_BEHAVIOUR = 12               # Philox stream of the behaviour head's exploration draws
BEHAVIOUR_NOISE_WORDS = 4           # fwg_behaviour_act's noise_params: sigma (float bits), eps_scaled low / high word, 0


class NativeError(RuntimeError):
    pass


INSTANCE_SHAPE = 1000       # include/fwgym.h FWG_INSTANCE_SHAPE: fwg_spec_index / fwg_config_instance values from here on are shape instances
INSTANCE_GENERIC = 100000   # FWG_INSTANCE_GENERIC (fwg_config_instance only)


_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libfwgym.so")
_vp, _i64, _u64, _int, _f32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_float
_cfg = C.POINTER(Config)
# every export of include/fwgym.h: name -> (restype, argtypes); handles, device pointers and streams are void pointers
PROTOTYPES = {
    "fwg_abi_version": (_int, []),
    "fwg_last_error": (C.c_char_p, []),
    "fwg_get_layout": (_int, [_cfg, C.POINTER(Layout)]),
    "fwg_create": (_int, [_cfg, _i64, _int, _vp, _i64, C.POINTER(_vp)]),
    "fwg_destroy": (_int, [_vp]),
    "fwg_update_config": (_int, [_vp, _cfg]),
    "fwg_seed": (_int, [_vp, _u64]),
    "fwg_global_step": (_i64, [_vp]),
    "fwg_reset": (_int, [_vp] * 6),
    "fwg_step": (_int, [_vp] * 10),
    "fwg_check_actions": (_int, [_vp, _vp, _vp]),
    "fwg_finish_episodes": (_int, [_vp, _vp, _vp]),
    "fwg_reduce_success": (_int, [_vp, C.POINTER(_f32), _vp]),
    "fwg_reduce_success_device": (_int, [_vp, _vp, _vp]),
    "fwg_dump_spec": (_int, [_cfg, C.POINTER(C.c_uint32), _i64]),
    "fwg_num_specs": (_int, []),
    "fwg_spec_index": (_int, [_vp]),
    "fwg_config_instance": (_int, [_cfg]),
    "fwg_set_graph_mode": (_int, [_vp, _int, _vp]),
    "fwg_note_replayed_steps": (_int, [_vp, _i64]),
    "fwg_capture_begin": (_int, [_vp]),
    "fwg_capture_end": (_int, [_vp]),
    "fwg_capture_parity": (_int, [_vp]),
    "fwg_replay_check": (_int, [_vp, _int]),
    "fwg_obs_log_floats": (_i64, [_cfg, _i64]),
    "fwg_obs_window": (_int, [_vp, C.POINTER(_i64)]),
    "fwg_obs_gather": (_int, [_vp] * 4),
    "fwg_gae": (_int, [_i64, _i64, _vp, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp]),
    "fwg_pid_act": (_int, [_i64, _vp, _int, C.POINTER(C.c_int32), _vp, _int, C.POINTER(C.c_int32), PidGains, _vp, _vp, _vp]),
    "fwg_eval_advance": (_int, [_i64, _i64] + [_vp] * 9 + [_i64, _vp, _vp]),
    "fwg_record_row_words": (_i64, []),
    "fwg_record_start": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _i64, _vp]),
    "fwg_record": (_int, [_vp, _vp, _int] + [_vp] * 6 + [_i64, _vp]),
    "fwg_monitor_scratch_bytes": (_i64, [_i64]),
    "fwg_monitor_fold": (_int, [_i64, _i64] + [_vp] * 6),
    "fwg_monitor_take": (_int, [_i64, _vp, _vp, _vp]),
    "fwg_goal_window": (_int, [_vp]),
    "fwg_goal_observe": (_int, [_vp, C.POINTER(GoalSpecStruct), _vp, _vp, _vp]),
    "fwg_goal_reward": (_int, [_vp, C.POINTER(GoalSpecStruct), _i64] + [_vp] * 7),
    "fwg_goal_relabel": (_int, [_vp, C.POINTER(GoalSpecStruct), _i64] + [_vp] * 5 + [_u64, C.c_uint32, _u64] + [_vp] * 4),
    "fwg_replay_index": (_int, [_i64, _i64, _vp, _vp, _vp]),
    "fwg_replay_sample": (_int, [_vp, C.POINTER(GoalSpecStruct), C.POINTER(ReplayView), _int, _i64, _u64, C.c_uint32, _u64] + [_vp] * 9),
    "fwg_selftest_philox": (_int, [_vp, _vp, _i64, _vp]),
    "fwg_actor_create": (_int, [_int, _i64, _int, _int, _f32, _f32, _f32, _f32, C.POINTER(_vp)]),
    "fwg_actor_destroy": (None, [_vp]),
    "fwg_actor_set_weights": (_int, [_vp, C.POINTER(ActorWeights)]),
    "fwg_actor_set_conv": (_int, [_vp, _int, _int, _vp, _vp]),
    "fwg_actor_set_stats": (_int, [_vp, C.POINTER(ActorStats), _vp]),
    "fwg_actor_get_stats": (_int, [_vp, C.POINTER(ActorStats), _vp]),
    "fwg_actor_configure": (_int, [_vp, _int, _int]),
    "fwg_actor_seed": (_int, [_vp, _u64, _i64]),
    "fwg_actor_observe": (_int, [_vp] * 5),
    "fwg_actor_act": (_int, [_vp] * 10 + [_int, _vp]),
    "fwg_actor_set_obs_log": (_int, [_vp, _vp]),
    "fwg_attach_observer": (_int, [_vp, _vp]),
    "fwg_rollout_available": (_int, [_vp, _vp]),
    "fwg_rollout_step": (_int, [_vp] * 14 + [_int, _vp]),
    "fwg_learner_create": (_int, [_vp, C.POINTER(_vp)]),
    "fwg_learner_create_cnn": (_int, [_vp, C.POINTER(_vp)]),
    "fwg_learner_destroy": (None, [_vp]),
    "fwg_learner_num_params": (_i64, [_vp]),
    "fwg_ppo_moments": (_int, [_vp, _vp, _vp, _i64, _int, _vp, _vp]),
    "fwg_ppo_grad": (_int, [_vp, C.POINTER(PpoBatch), _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "fwg_ppo_apply": (_int, [_vp, _vp, _i64] + [_vp] * 7),
    "fwg_ppo_step": (_int, [_vp, C.POINTER(PpoBatch), _vp, _i64] + [_vp] * 8),
    "fwg_actor_pack": (_int, [_vp, _vp, _vp]),
    "fwg_offpolicy_create": (_int, [_int, _int, _int, _int, C.POINTER(_vp)]),
    "fwg_offpolicy_destroy": (None, [_vp]),
    "fwg_offpolicy_num_params": (_i64, [_vp]),
    "fwg_offpolicy_actor_params": (_i64, [_vp]),
    "fwg_ddpg_critic_grad": (_int, [_vp, C.POINTER(OffpolicyBatch), _i64, C.POINTER(DdpgHparams)] + [_vp] * 5),
    "fwg_ddpg_actor_grad": (_int, [_vp, C.POINTER(OffpolicyBatch), _i64, _vp, _vp, _vp]),
    "fwg_ddpg_apply": (_int, [_vp, _int, _vp, _i64, C.POINTER(DdpgHparams)] + [_vp] * 7),
    "fwg_ddpg_step": (_int, [_vp, C.POINTER(OffpolicyBatch), _i64, _i64, _int, C.POINTER(DdpgHparams)] + [_vp] * 7),
    "fwg_behaviour_act": (_int, [_vp, C.POINTER(GoalSpecStruct), _i64, _int, _int, _int] + [_vp] * 11 + [_u64, C.c_uint32, _int, _vp]),
}
EXPORTS = list(PROTOTYPES)
_libs = {}


def load_library(path=None):
    """Loads libfwgym.so and declares the prototypes.  Raises NativeError when the library is missing: build it with
    `python __graft_entry__.py` (or `make -C fixed-wing-gym_amd`)."""
    path = os.path.abspath(path or os.environ.get("FWGYM_LIB", DEFAULT_LIB))
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise NativeError("HIP library {} not found: build it first (python -c 'import __graft_entry__ as g; "
                          "g.build()'); there is no CPU fallback".format(path))
    try:
        # PyTorch-ROCm bundles its own HIP runtime; it must be the one already mapped when libfwgym.so resolves
        # libamdhip64, otherwise the process ends up with two runtimes and no visible device
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            raise NativeError("{} does not export {}".format(path, name))
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.fwg_abi_version() != FWG_ABI_VERSION:
        raise NativeError("ABI mismatch: library {} vs binding {}".format(lib.fwg_abi_version(), FWG_ABI_VERSION))
    _libs[path] = lib
    return lib


def check(lib, status):
    if status != 0:
        msg = lib.fwg_last_error().decode("utf-8", "replace")
        if status == -4:
            raise AssertionError(msg)  # NaN action: the reference asserts (fixed_wing.py:347)
        raise NativeError("libfwgym error {}: {}".format(status, msg))
