"""ctypes mirror of include/adrp.h (struct layouts and constants).

Must stay byte-identical with the header: tests/test_abi.py checks sizeof() against the
value adrp_default_config() writes into ``struct_size``.
"""
import ctypes

ABI_VERSION = 2
MAX_DRONES = 8
MAX_GATES = 4
MAX_OBSTACLES = 4

OK, ERR_INVALID, ERR_DEVICE, ERR_OOM = 0, -1, -2, -3

TASK_HOVER, TASK_RACE, TASK_MULTIHOVER, TASK_CTRL, TASK_VELOCITY = 0, 1, 2, 3, 4
PHYS_PYB, PHYS_DYN, PHYS_PYB_GND, PHYS_PYB_DRAG, PHYS_PYB_DW, PHYS_PYB_GND_DRAG_DW = range(6)
ACT_RPM, ACT_ONE_D_RPM, ACT_FULLSTATE, ACT_PID, ACT_VEL, ACT_ONE_D_PID, ACT_RAW_RPM = 0, 1, 2, 3, 4, 5, 6
MATH_RCP, MATH_RSQ, MATH_SQRT, MATH_SIN_SMALL, MATH_COS_SMALL, MATH_ATAN2, MATH_ASIN, MATH_EXP = range(8)   # adrp_math_probe
MATH_SQRT_NN, MATH_RCP_NC, MATH_RSQ_NC, MATH_SIN_TINY, MATH_COS_TINY = 8, 9, 10, 11, 12
MATH_EXPMAP_SINC, MATH_EXPMAP_COS, MATH_QUAT_INV_NORM, MATH_NORMAL_Z0, MATH_NORMAL_Z1 = 13, 14, 15, 16, 17
MATH_DIVC, MATH_SIN_FAST, MATH_COS_FAST = 18, 19, 20
MATH_EXP_TAB, MATH_ATAN2_NC, MATH_FDIV_RCP = 21, 22, 23
(MATHV_EULER_XYZ, MATHV_EULER_XYZ_FAST, MATHV_EULER_XYZ_FAST_U, MATHV_QUAT_FROM_EULER, MATHV_QUAT_FROM_EULER_FAST,
 MATHV_FATAN2, MATHV_FASIN, MATHV_FEXP, MATHV_SMALL_SINCOS, MATHV_EXPMAP_SINC_COS, MATHV_QUAT_INV_NORM,
 MATHV_CLAMP100_WV) = range(12)   # adrp_math_probe_v
MATHV_PLANES = {MATHV_EULER_XYZ: (4, 3), MATHV_EULER_XYZ_FAST: (4, 3), MATHV_EULER_XYZ_FAST_U: (4, 3),
                MATHV_QUAT_FROM_EULER: (3, 4), MATHV_QUAT_FROM_EULER_FAST: (3, 4), MATHV_FATAN2: (2, 1), MATHV_FASIN: (1, 1),
                MATHV_FEXP: (1, 1), MATHV_SMALL_SINCOS: (1, 2), MATHV_EXPMAP_SINC_COS: (1, 2), MATHV_QUAT_INV_NORM: (1, 1),
                MATHV_CLAMP100_WV: (6, 6)}   # (input planes, output planes)
RACE_COMPARE, RACE_COMPETE = 0, 1
POLICY_TANH, POLICY_RELU = 0, 1
POLICY_RAW, POLICY_RELATIVE, POLICY_ABSOLUTE = 0, 1, 2
VEC_SLOTS = 4   # ADRP_VEC_SLOTS
DSLPID_CF2X, DSLPID_CF2P = 0, 1
CMD_NF, CMD_NI, CMD_ARGS = 63, 3, 14   # ADRP_CMD_NF / _NI / _ARGS (command state, adrp_mellinger_*)
RACE_CTRL_NONE, RACE_CTRL_HARDCODED, RACE_CTRL_POLICY = 0, 1, 2

_d = ctypes.c_double
_i32 = ctypes.c_int32


def _arr(t, *dims):
    for n in reversed(dims):
        t = t * n
    return t


class AdrpDroneParams(ctypes.Structure):
    _fields_ = [
        ("m", _d), ("l", _d), ("thrust2weight", _d),
        ("ixx", _d), ("iyy", _d), ("izz", _d),
        ("kf", _d), ("km", _d),
        ("collision_h", _d), ("collision_r", _d), ("collision_z_offset", _d),
        ("max_speed_kmh", _d),
        ("gnd_eff_coeff", _d), ("prop_radius", _d),
        ("drag_coeff", _arr(_d, 3)),
        ("dw_coeff", _arr(_d, 3)),
        ("prop_pos", _arr(_d, 4, 3)),
    ]


class AdrpTrack(ctypes.Structure):
    _fields_ = [
        ("num_gates", _i32), ("num_obstacles", _i32),
        ("gates", _arr(_d, MAX_GATES, 7)),
        ("obstacles", _arr(_d, MAX_OBSTACLES, 6)),
        ("bounds_hi", _arr(_d, 3)),
        ("episode_len_sec", _d),
        ("random_gates_obstacles", _i32),
        ("gate_offset_range", _arr(_d, 2)),
        ("obstacle_offset_range", _arr(_d, 2)),
        ("random_drone_state", _i32),
        ("pos_offset_range", _arr(_d, 3, 2)),
        ("rot_offset_range", _arr(_d, 3, 2)),
        ("random_drone_inertia", _i32),
        ("inertia_offset_range", _arr(_d, 4, 2)),
        ("disturbances", _i32),
        ("action_noise_std", _d),
        ("dyn_dist_low", _arr(_d, 3)), ("dyn_dist_high", _arr(_d, 3)),
        ("init_pos", _arr(_d, MAX_DRONES, 3)),
        ("init_vel", _arr(_d, MAX_DRONES, 3)),
        ("init_rpy", _arr(_d, MAX_DRONES, 3)),
        ("init_pqr", _arr(_d, MAX_DRONES, 3)),
        ("race_mass", _d),
        ("race_inertia", _arr(_d, 3)),
        ("reward_wrapper", _i32),
        ("obs_wrapper", _i32),
    ]


class AdrpConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("task", _i32), ("physics", _i32), ("act_type", _i32), ("race_mode", _i32),
        ("num_envs", _i32), ("num_drones", _i32),
        ("pyb_freq", _i32), ("ctrl_freq", _i32),
        ("action_buffer_size", _i32),
        ("autoreset", _i32),
        ("precision", _i32),
        ("link_frame_lag", _i32),
        ("env_offset", ctypes.c_int64),
        ("seed", ctypes.c_uint64),
        ("gravity", _d),
        ("drone", AdrpDroneParams),
        ("init_xyz", _arr(_d, MAX_DRONES, 3)),
        ("init_rpy", _arr(_d, MAX_DRONES, 3)),
        ("init_xyz_noise", _arr(_d, 3)),
        ("init_rpy_noise", _arr(_d, 3)),
        ("init_vel_noise", _arr(_d, 3)),
        ("init_omega_noise", _arr(_d, 3)),
        ("target_pos", _arr(_d, 3)),
        ("episode_len_sec", _d),
        ("track", AdrpTrack),
    ]

    def copy(self):
        c = AdrpConfig()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(self), ctypes.sizeof(self))
        return c


def set_vec(arr, values):
    """Assign a (nested) python sequence into a ctypes array in place."""
    for k, v in enumerate(values):
        if hasattr(arr[k], "__len__") and not isinstance(arr[k], (int, float)):
            set_vec(arr[k], v)
        else:
            arr[k] = v


def to_list(arr):
    out = []
    for x in arr:
        out.append(to_list(x) if hasattr(x, "__len__") else x)
    return out


class AdrpVecIO(ctypes.Structure):
    """adrp_vec_io (include/adrp.h): one host block of the SB3 host path (adrp_vec_bind)"""
    _p = ctypes.c_void_p
    _fields_ = [("act", _p), ("obs", _p), ("rew", _p), ("term", _p), ("trunc", _p), ("done", _p),
                ("count", _p), ("idx", _p), ("rows", _p), ("cap", ctypes.c_int),
                ("term_dev", _p), ("trunc_dev", _p), ("tobs_dev", _p), ("idx_dev", _p)]


class AdrpPpoCfg(ctypes.Structure):
    """adrp_ppo_cfg (include/adrp.h): the constants of PPOLearner's minibatch update"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("normalize_advantage", _i32),
                ("learning_rate", _d), ("clip_range", _d), ("clip_range_vf", _d),
                ("ent_coef", _d), ("vf_coef", _d), ("max_grad_norm", _d)]


class AdrpDslpidParams(ctypes.Structure):
    """adrp_dslpid_params (include/adrp.h): gains, mixer and model constants of the stand-alone DSLPIDControl"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", _i32),
                ("p_for", _arr(_d, 3)), ("i_for", _arr(_d, 3)), ("d_for", _arr(_d, 3)),
                ("p_tor", _arr(_d, 3)), ("i_tor", _arr(_d, 3)), ("d_tor", _arr(_d, 3)),
                ("mixer", _arr(_d, 4, 3)),
                ("gravity", _d), ("kf", _d),
                ("pwm2rpm_scale", _d), ("pwm2rpm_const", _d), ("min_pwm", _d), ("max_pwm", _d)]


class AdrpEpisodeIO(ctypes.Structure):
    """adrp_episode_io (include/adrp.h): the caller-owned device buffers of the on-device episode statistics"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("capacity", _i32), ("ring", _i32),
                ("quota", _p), ("run_return", _p), ("run_length", _p), ("count", _p), ("meta", _p),
                ("log_return", _p), ("log_length", _p), ("log_env", _p)]


class AdrpRaceCtrlIO(ctypes.Structure):
    """adrp_race_ctrl_io (include/adrp.h): the caller-owned device buffers of the race evaluation's controller launch"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("num_drones", _i32), ("ref_len", _i32),
                ("kind", _arr(_i32, MAX_DRONES)),
                ("ref", _p), ("offset", _p), ("phase", _p), ("setpoints", _p), ("codes", _p), ("args", _p)]


class AdrpRaceResultsIO(ctypes.Structure):
    """adrp_race_results_io (include/adrp.h): the caller-owned device buffers of the per-drone race results"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("num_drones", _i32), ("capacity", _i32),
                ("base", _i32), ("reserved", _i32),
                ("open", _p), ("run_return", _p), ("run_length", _p), ("gates", _p), ("finish", _p), ("elim", _p),
                ("meta", _p), ("log_return", _p), ("log_length", _p), ("log_term", _p), ("log_trunc", _p),
                ("log_gates", _p), ("log_finish", _p), ("log_elim", _p)]


AGENTS_OBS_MIN = 49                                    # ADRP_AGENTS_OBS_MIN


class AdrpRaceAgentsIO(ctypes.Structure):
    """adrp_race_agents_io (include/adrp.h): the caller-owned device buffers of the per-drone race agents"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("num_drones", _i32), ("obs_dim", _i32),
                ("num_gates", _i32), ("reserved", _i32),
                ("wr_gate", _p), ("wr_target", _p), ("wr_prev", _p), ("alive", _p), ("run_return", _p), ("run_length", _p)]


ROSTER_NONE, ROSTER_HARDCODED, ROSTER_POLICY, ROSTER_LEARNER = 0, 1, 2, 3   # ADRP_ROSTER_* (the first three: RACE_CTRL_*)


class AdrpRaceRosterIO(ctypes.Structure):
    """adrp_race_roster_io (include/adrp.h): the roster and the caller-owned device buffers of the roster collector"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("num_drones", _i32), ("num_learners", _i32),
                ("ref_len", _i32), ("reserved", _i32), ("ctrl_freq", _d),
                ("role", _arr(_i32, MAX_DRONES)), ("learner_index", _arr(_i32, MAX_DRONES)),
                ("clock", _p), ("phase", _p), ("ref", _p), ("offset", _p), ("setpoints", _p), ("learner_act", _p),
                ("codes", _p), ("args", _p)]


PLAN_KNOTS, PLAN_COEF, PLAN_OBS_MIN = 20, 16, 28       # ADRP_PLAN_*
PLAN_NOT_IER0, PLAN_CEILING = 1, 2                     # adrp_race_plan status bits 0 / 1; n in bits 8..15, iterations 16..23


class AdrpRacePlanIO(ctypes.Structure):
    """adrp_race_plan_io (include/adrp.h): the caller-owned device buffers of the scripted racer's spline planner"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("num_drones", _i32), ("ref_len", _i32),
                ("obs_stride", _i32), ("reserved", _i32),
                ("obs", _p), ("mask", _p), ("samples", _p), ("ref", _p), ("status", _p),
                ("knots", _p), ("n_knots", _p), ("coef", _p), ("phase", _p)]


class AdrpRaceCameraIO(ctypes.Structure):
    """adrp_race_camera_io (include/adrp.h): the scene, the state planes and the caller-owned images of the drone camera"""
    _p = ctypes.c_void_p
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_envs", _i32), ("num_drones", _i32), ("width", _i32),
                ("height", _i32), ("num_gates", _i32), ("num_obstacles", _i32), ("gate_low", _arr(_i32, 4)),
                ("precision", _i32), ("capture_freq", _i32), ("reserved", _i32),
                ("pos", _p), ("quat", _p), ("gates", _p), ("obstacles", _p), ("step_counter", _p), ("mask", _p),
                ("dep", _p), ("seg", _p), ("rgb", _p)]
