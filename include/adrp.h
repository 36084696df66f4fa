/*
 * adrp.h — C-ABI of the MI355X-native batched quadrotor step (libadrp.so).
 *
 * One handle = one batch of E independent envs x N drones resident in the HBM of one
 * GPU.  Every pointer argument named *_dev is a DEVICE pointer (e.g. a torch tensor's
 * data_ptr() on the same GPU); `stream` is a hipStream_t (NULL = default stream).
 * All calls are stream-ordered and asynchronous; none of them synchronises the host
 * except adrp_create / adrp_destroy.  Return codes: ADRP_OK (0) or a negative
 * ADRP_ERR_*; nothing throws across the ABI.  adrp_last_error() gives the text.
 *
 * Reference interfaces replaced (file:line into FelixWaiblinger/gym-pybullet-adrp
 * snapshot 2024-10-08):
 *   adrp_create  <- BaseAviary.__init__            envs/BaseAviary.py:25-219
 *                   HoverAviary.__init__           envs/HoverAviary.py:11-64
 *                   MultiRaceAviary.__init__       envs/MultiRaceAviary.py:31-123
 *                   (+ the controller processes    envs/MultiRaceAviary.py:107-115)
 *   adrp_reset   <- BaseAviary.reset               envs/BaseAviary.py:223-258
 *                   MultiRaceAviary.reset          envs/MultiRaceAviary.py:127-167
 *   adrp_step    <- BaseAviary.step                envs/BaseAviary.py:262-387
 *                   MultiRaceAviary.step           envs/MultiRaceAviary.py:171-270
 *                   (+ MellingerControl.computeControl control/MellingerControl.py:154-262
 *                    + RewardWrapper._compute_reward utils/wrapper.py:121-186)
 *   adrp_get_state / adrp_set_state
 *                <- p.getBasePositionAndOrientation / p.resetBasePositionAndOrientation /
 *                   p.getBaseVelocity / p.resetBaseVelocity (BaseAviary.py:520-523,
 *                   MultiRaceAviary.py:456-467): state snapshot / teacher forcing
 *   adrp_destroy <- BaseAviary.close / MultiRaceAviary.close
 *                   envs/BaseAviary.py:420-425, envs/MultiRaceAviary.py:274-280
 */
#ifndef ADRP_H
#define ADRP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADRP_ABI_VERSION 2

#define ADRP_MAX_DRONES 8
#define ADRP_MAX_GATES 4      /* MultiRaceAviary._computeObs hard-codes 4 (MultiRaceAviary.py:591-651) */
#define ADRP_MAX_OBSTACLES 4

/* status codes */
#define ADRP_OK 0
#define ADRP_ERR_INVALID (-1)   /* bad argument / config (cf. ValueError, BaseAviary.py:79-80) */
#define ADRP_ERR_DEVICE (-2)    /* HIP runtime error */
#define ADRP_ERR_OOM (-3)       /* device allocation failed */

/* adrp_config.task */
#define ADRP_TASK_HOVER 0       /* HoverAviary (envs/HoverAviary.py) */
#define ADRP_TASK_RACE 1        /* MultiRaceAviary (envs/MultiRaceAviary.py) */
/* MultiHoverAviary (envs/MultiHoverAviary.py): num_drones 1..8 drones per env, RPM / ONE_D_RPM actions.
 * The config is HoverAviary's with num_drones and init_xyz[n] / init_rpy[n] per drone; the targets are
 * derived, TARGET_POS[n] = init_xyz[n] + (0, 0, 1/(n+1)) (MultiHoverAviary.py:71), target_pos is ignored.
 * obs [E,N,12+B*A], action [E,N,A], reward / terminated / truncated [E] (sums / any over the env's
 * drones, bounds 2.0); an env's drones reset together and the action ring of a reset env is cleared.
 * Snapshot: HoverAviary's fields, [field][E*N], column e*N+n; the per-env ints (step_counter, episode,
 * ring_head) are replicated on the env's columns and adrp_set_state takes drone 0's. */
#define ADRP_TASK_MULTIHOVER 2
/* CtrlAviary (envs/CtrlAviary.py) and VelocityAviary (envs/VelocityAviary.py): the control-application
 * envs, num_drones 1..8 per env.  The observation is the drone state row of _getDroneStateVector
 * (BaseAviary.py:553-573), float [E,N,20] = pos 3, quat 4 (xyzw), rpy 3, vel 3, ang_v 3 and the four
 * RPMs applied in this step (zero after a reset); the action is float [E,N,4]: motor speeds clipped to
 * [0, MAX_RPM] (CTRL, act_type ADRP_ACT_RAW_RPM; adrp_step_rpm takes them in the handle's precision)
 * or a velocity command (direction 3, fraction of SPEED_LIMIT 1) tracked by one DSLPIDControl per
 * drone, called once per step before the sub-steps (VELOCITY, act_type ADRP_ACT_VEL).  reward -1,
 * terminated / truncated 0, always: action_buffer_size and autoreset are ignored.  The downwash
 * physics modes couple an env's drones as in MULTIHOVER.  Snapshot: HoverAviary's base fields without
 * ring fields, [field][E*N], column e*N+n, last_rpm_* maintained in every physics mode; VELOCITY adds
 * the nine pid_* fields, which adrp_reset leaves as they are (the reference builds its controllers
 * once).  The ints are per column; adrp_set_state takes drone 0's for the env. */
#define ADRP_TASK_CTRL 3
#define ADRP_TASK_VELOCITY 4

/* adrp_config.physics — utils/enums.py:18-26 (Physics) */
#define ADRP_PHYS_PYB 0
#define ADRP_PHYS_DYN 1
#define ADRP_PHYS_PYB_GND 2
#define ADRP_PHYS_PYB_DRAG 3
#define ADRP_PHYS_PYB_DW 4
#define ADRP_PHYS_PYB_GND_DRAG_DW 5

/* adrp_config.act_type — utils/enums.py:40-47 (ActionType) */
#define ADRP_ACT_RPM 0          /* HoverAviary: a in [-1,1]^4 -> HOVER_RPM*(1+0.05a) (BaseRLAviary.py:192) */
#define ADRP_ACT_ONE_D_RPM 1    /* HoverAviary: a in [-1,1]   -> 4 x HOVER_RPM*(1+0.05a) (BaseRLAviary.py:225) */
#define ADRP_ACT_FULLSTATE 2    /* MultiRace: [x,y,z,yaw] absolute FULLSTATE setpoint (MultiRaceAviary.py:190-194) */
/* HoverAviary with the fused DSLPIDControl (control/DSLPIDControl.py:82-259), once per env.step */
#define ADRP_ACT_PID 3          /* a in R^3: waypoint, capped 1 m away (BaseRLAviary.py:193-207, BaseAviary.py:1112-1160) */
#define ADRP_ACT_VEL 4          /* a in R^4: direction + |a3| x SPEED_LIMIT target velocity (BaseRLAviary.py:208-223) */
#define ADRP_ACT_ONE_D_PID 5    /* a in R:   target z = z + 0.1a (BaseRLAviary.py:226-235) */
#define ADRP_ACT_RAW_RPM 6      /* CtrlAviary: a in R^4, motor speeds, clipped to [0, MAX_RPM] (CtrlAviary.py:140) */

/* adrp_config.race_mode — utils/enums.py:84-87 (RaceMode) */
#define ADRP_RACE_COMPARE 0
#define ADRP_RACE_COMPETE 1

/* High-level commands: utils/enums.py:58-70 (Command), as MultiRaceAviary.step sends them to
 * each drone's MellingerControl (envs/MultiRaceAviary.py:190-210, control/MellingerControl.py:17-61).
 * adrp_race_command args: ADRP_CMD_ARGS float64 per drone.  Slots 0..12 hold the command's own
 * arguments, flattened in the reference's order; slot 13 holds the reference's args[-1], which
 * low_level_control hands to process_command_queue as the commander clock (MellingerControl.py:57,
 * 292-303) — for FULLSTATE that is its timestep, for TAKEOFF [h, d] it is d. */
#define ADRP_CMD_NONE 0         /* ignored (low_level_control: else -> continue) */
#define ADRP_CMD_FULLSTATE 1    /* pos[3], vel[3], acc[3], yaw, rpy_rate[3]            (491-543) */
#define ADRP_CMD_TAKEOFF 2      /* height, duration                                    (547-561) */
#define ADRP_CMD_TAKEOFFYAW 3   /* height, duration, yaw                               (565-580) */
#define ADRP_CMD_TAKEOFFVEL 4   /* height, velocity, relative                          (584-599) */
#define ADRP_CMD_LAND 5         /* height, duration                                    (603-617) */
#define ADRP_CMD_LANDYAW 6      /* height, duration, yaw                               (621-636) */
#define ADRP_CMD_LANDVEL 7      /* height, velocity, relative                          (640-655) */
#define ADRP_CMD_STOP 8         /* -                                                   (659-668) */
#define ADRP_CMD_GOTO 9         /* x, y, z, yaw, duration, relative                    (672-689) */
#define ADRP_CMD_NOTIFY 10      /* - (notifySetpointStop)                              (691-699) */
#define ADRP_CMD_ARGS 14
#define ADRP_CMD_TIME_SLOT 13
/* Per-drone command state (adrp_get_command_state), float fields then int32 fields, each a
 * contiguous [E*N] vector like adrp_get_state's.  Floats: setpoint_t position 3, velocity 3,
 * acceleration 3, attitudeRate 3 [deg/s], attitudeQuaternion z, w (FULLSTATE), attitude.yaw [deg]
 * (commander); the commander's pos 3, vel 3, yaw [rad]; state_t position 3, velocity 3,
 * attitude.yaw [deg] of the last _update_state; planner t_begin, duration, 4 x 8 polynomial
 * coefficients (x, y, z, yaw).  Ints: planner state (0 idle, 1 flying, 2 landing),
 * full_state_cmd_override, setpoint mode (0 never set, 1 FULLSTATE, 2 commander). */
#define ADRP_CMD_NF 63
#define ADRP_CMD_NI 3

/* Drone constants, as BaseAviary._parseURDFParameters reads them (BaseAviary.py:989-1021). */
typedef struct adrp_drone_params {
    double m;                  /* base mass [kg] */
    double l;                  /* arm [m] */
    double thrust2weight;
    double ixx, iyy, izz;      /* diagonal inertia [kg m^2] */
    double kf, km;             /* thrust / torque coefficients */
    double collision_h, collision_r, collision_z_offset;
    double max_speed_kmh;
    double gnd_eff_coeff, prop_radius;
    double drag_coeff[3];      /* xy, xy, z */
    double dw_coeff[3];
    double prop_pos[4][3];     /* prop link COM in the body frame (URDF inertial origins) */
} adrp_drone_params;

/* MultiRace track / randomisation description: the YAML schema of config/level*.yaml. */
typedef struct adrp_track {
    int32_t num_gates;                               /* <= ADRP_MAX_GATES */
    int32_t num_obstacles;                           /* <= ADRP_MAX_OBSTACLES */
    double gates[ADRP_MAX_GATES][7];                 /* nominal x,y,z,r,p,y,type(0 tall,1 low) */
    double obstacles[ADRP_MAX_OBSTACLES][6];         /* nominal x,y,z,r,p,y */
    double bounds_hi[3];                             /* |pos| > bounds[1] eliminates (MultiRaceAviary.py:684) */
    double episode_len_sec;
    int32_t random_gates_obstacles;
    double gate_offset_range[2];                     /* U(lo,hi) on x,y,yaw */
    double obstacle_offset_range[2];                 /* U(lo,hi) on x,y */
    int32_t random_drone_state;
    double pos_offset_range[3][2];                   /* U ranges x,y,z */
    double rot_offset_range[3][2];                   /* U ranges r,p,y */
    int32_t random_drone_inertia;
    double inertia_offset_range[4][2];               /* U ranges on M, Ixx, Iyy, Izz */
    int32_t disturbances;
    double action_noise_std;                         /* N(0,std) thrust noise per motor per sub-step */
    double dyn_dist_low[3], dyn_dist_high[3];        /* U(low,high) world force per drone per sub-step */
    double init_pos[ADRP_MAX_DRONES][3];             /* config init_states.droneK.pos */
    double init_vel[ADRP_MAX_DRONES][3];
    double init_rpy[ADRP_MAX_DRONES][3];             /* raw config value */
    double init_pqr[ADRP_MAX_DRONES][3];
    double race_mass;                                /* cf2x.urdf base mass used by changeDynamics (0.027) */
    double race_inertia[3];
    int32_t reward_wrapper;                          /* 0: env reward (0, MultiRaceAviary.py:665-670);
                                                        1: RewardWrapper (utils/wrapper.py:121-186) */
    int32_t obs_wrapper;                             /* DroneObservationWrapper (utils/wrapper.py:38-65):
                                                        yaw actions forced to 0, terminated once drone 0's
                                                        current gate >= 2.  0: off; 1: inside the
                                                        RewardWrapper (its terminal terms see the early
                                                        termination); 2: outside it */
} adrp_track;

typedef struct adrp_config {
    uint32_t struct_size;      /* = sizeof(adrp_config); checked by adrp_create */
    int32_t task;              /* ADRP_TASK_* */
    int32_t physics;           /* ADRP_PHYS_* */
    int32_t act_type;          /* ADRP_ACT_* */
    int32_t race_mode;         /* ADRP_RACE_* */
    int32_t num_envs;          /* E (envs on THIS device) */
    int32_t num_drones;        /* N drones per env */
    int32_t pyb_freq;          /* physics Hz (must be a multiple of ctrl_freq) */
    int32_t ctrl_freq;         /* env.step Hz */
    int32_t action_buffer_size;/* HoverAviary obs action ring (ctrl_freq//2, BaseRLAviary.py:66) */
    int32_t autoreset;         /* 1: done envs are reset inside adrp_step (VecEnv semantics) */
    int32_t precision;         /* 0 = fp32 kernel, 1 = fp64 kernel */
    int32_t link_frame_lag;    /* 1 (pybullet): LINK_FRAME forces/torques on links are rotated by the
                                  link transform cached at the last forwardKinematics, i.e. the pose
                                  at the start of the previous stepSimulation */
    int64_t env_offset;        /* global id of local env 0 (RNG key; multi-GPU sharding) */
    uint64_t seed;
    double gravity;            /* G = 9.8 (BaseAviary.py:74) */
    adrp_drone_params drone;
    /* HoverAviary */
    double init_xyz[ADRP_MAX_DRONES][3];   /* INIT_XYZS (BaseAviary.py:194-199) */
    double init_rpy[ADRP_MAX_DRONES][3];   /* INIT_RPYS [rad] */
    double init_xyz_noise[3];              /* extension: U(-n,n) added per reset (0 = reference) */
    double init_rpy_noise[3];
    double init_vel_noise[3];
    double init_omega_noise[3];
    double target_pos[3];                  /* HoverAviary.TARGET_POS (HoverAviary.py:51) */
    double episode_len_sec;                /* HoverAviary.EPISODE_LEN_SEC (HoverAviary.py:52) */
    /* MultiRaceAviary */
    adrp_track track;
} adrp_config;

typedef struct adrp_handle adrp_t;

/* ABI version of the loaded library (must equal ADRP_ABI_VERSION). */
int adrp_abi_version(void);

/* Fill *cfg with the reference defaults for `task` (HoverAviary, MultiRaceAviary or MultiHoverAviary,
 * CF2X = cf2x_IROS.urdf constants, level0 track for RACE; MULTIHOVER: the hover default with two
 * drones at init_xyz[n] = (4Ln, 4Ln, COLLISION_H/2 - COLLISION_Z_OFFSET + 0.1), BaseAviary.py:194-197;
 * CTRL / VELOCITY: the hover default with one drone at 240 / 240 Hz (CtrlAviary.py:19-20,
 * VelocityAviary.py:21-22), act_type RAW_RPM / VEL, and init_xyz[n] of that formula for all eight n). */
int adrp_default_config(int task, adrp_config* cfg);

/* Create a handle on GPU `device`; allocates all state in HBM. */
int adrp_create(const adrp_config* cfg, int device, adrp_t** out);
void adrp_destroy(adrp_t* h);

/* Error text of the last failing call on h (h may be NULL for adrp_create failures). */
const char* adrp_last_error(const adrp_t* h);

/* Per-drone observation width D (12 + B*A for Hover: 72 RPM/VEL, 57 PID, 27 ONE_D_*;
 * 49 / 49+6(N-1) Race; 20 CtrlAviary / VelocityAviary) and action width A (4, 3 or 1). */
int adrp_obs_dim(const adrp_t* h);
int adrp_act_dim(const adrp_t* h);

/* Re-key the handle's random streams (reset randomisation, level1-3 disturbances) as a fresh
 * handle created with `seed` has them: sets the seed and zeroes every env's episode counter
 * (stream-ordered).  Follow it with a full adrp_reset, as BaseAviary.reset(seed=...) reseeds and
 * resets (envs/BaseAviary.py:223-258).  A captured graph keeps the seed it was captured with. */
int adrp_reseed(adrp_t* h, uint64_t seed, void* stream);

/* MultiRaceAviary only: switch the RewardWrapper / DroneObservationWrapper fused into the step
 * (adrp_track.reward_wrapper / .obs_wrapper) on an existing handle, as wrapping the reference env
 * with RewardWrapper(env) / DroneObservationWrapper(env) does (utils/wrapper.py).  Synchronises. */
int adrp_set_wrappers(adrp_t* h, int reward_wrapper, int obs_wrapper);

/* Reset the envs selected by env_mask_dev (uint8 [E], NULL = all) and write their
 * observations into obs_dev (float [E,N,D]); rows of unselected envs are left as is. */
int adrp_reset(adrp_t* h, const uint8_t* env_mask_dev, float* obs_dev, void* stream);

/* One env.step() of every env: act_dev float [E,N,A] -> obs_dev [E,N,D],
 * rew_dev float [E], term_dev / trunc_dev uint8 [E].  With autoreset, envs whose
 * episode ended are reset in the same launch; their final observation is written to
 * terminal_obs_dev [E,N,D] (only those rows) when it is non-NULL, and obs_dev holds
 * the reset observation (SB3 VecEnv semantics). */
int adrp_step(adrp_t* h, const float* act_dev, float* obs_dev, float* rew_dev,
              uint8_t* term_dev, uint8_t* trunc_dev, float* terminal_obs_dev, void* stream);

/* ADRP_TASK_CTRL only: adrp_step with the motor speeds rpm_dev [E,N,4] in the handle's own precision
 * (float32 for precision 0, float64 for precision 1).  The reference feeds float64 RPMs; rounding them
 * to float32 first costs about 3e-5 relative in the velocity after one step, so a float64 handle that
 * is to follow the reference to 1e-9 takes them here.  adrp_step with float32 RPMs stays valid. */
int adrp_step_rpm(adrp_t* h, const void* rpm_dev, float* obs_dev, float* rew_dev,
                  uint8_t* term_dev, uint8_t* trunc_dev, void* stream);

/* MultiRaceAviary only: high-level command mode.  adrp_enable_commands
 * allocates the per-drone setpoint / commander / planner state; call it before the adrp_reset that
 * starts the episodes (envs already running start from an idle planner and an unset setpoint).
 * From then on adrp_step runs the step kernel that evaluates the commander's trajectory at every
 * controller call (MellingerControl._update_setpoint, MellingerControl.py:369-374).
 * adrp_race_command applies one command per drone (cmd_dev int32 [E,N] ADRP_CMD_*, args_dev float64
 * [E,N,ADRP_CMD_ARGS]) as the controller processes MultiRaceAviary.step's command message before the
 * sub-steps; eliminated drones get STOP (MultiRaceAviary.py:198-199).  Follow it with
 * adrp_step(h, NULL, ...), which keeps the setpoints the commands left.  adrp_step with a non-NULL
 * act_dev sends FULLSTATE (act[:3], 0, 0, act[3], 0, step_counter) first, as the ndarray path does
 * (MultiRaceAviary.py:190-194).  Parity of the commander is unpinned. */
int adrp_enable_commands(adrp_t* h);
int adrp_race_command(adrp_t* h, const int32_t* cmd_dev, const double* args_dev, void* stream);
/* float [ADRP_CMD_NF][E*N] (float32 at every precision), int32 [ADRP_CMD_NI][E*N] */
int adrp_get_command_state(adrp_t* h, float* f_dev, int32_t* i_dev, void* stream);
int adrp_set_command_state(adrp_t* h, const float* f_dev, const int32_t* i_dev, void* stream);

/* Snapshot layout: nf float fields and ni int32 fields, each field a contiguous
 * [E*N] vector (drone-major within env: index e*N+n).  Field names: adrp_state_field. */
int adrp_state_layout(const adrp_t* h, int* nf, int* ni);
const char* adrp_state_field(const adrp_t* h, int is_int, int index);
/* f_dev elements are float32 for precision 0 and float64 for precision 1. */
int adrp_get_state(adrp_t* h, void* f_dev, int32_t* i_dev, void* stream);
int adrp_set_state(adrp_t* h, const void* f_dev, const int32_t* i_dev, void* stream);

/* Name of the step-kernel instantiation a config selects (no device needed), e.g.
 * "hover_step<f32,PYB,A4,B15,cf2x>": "cf2x" = per-config constants compiled in (the
 * reference default drone at 240/30 Hz, chosen only when the config's derived constants
 * are bit-identical), "generic" = read from the handle's device-resident block.
 * MultiHoverAviary: "multihover_step<f32,PYB,A4,G2>", G = the lane-group width, the next power of two
 * >= num_drones (one lane per drone, a group per env).  CtrlAviary / VelocityAviary:
 * "ctrl_step<f64,PYB_DW,G4>" / "velocity_step<f64,PYB_DW,G4>". */
const char* adrp_kernel_name(const adrp_config* cfg);
/* the instantiation this handle launches now (after adrp_enable_commands a race handle runs the
   command-mode kernel, "...,CMD>"; ADRP_RACE_QUAD as read at create) */
const char* adrp_handle_kernel_name(const adrp_t* h);

/* Algorithmic HBM bytes one adrp_step moves (roofline accounting). */
int64_t adrp_step_bytes(const adrp_t* h);

/* Kernel timing with HIP events attached to the step kernel's own dispatch
 * (hipExtLaunchKernelGGL start/stop events): after adrp_profile_begin(h, n) the next n
 * adrp_step launches are timed; adrp_profile_end synchronises and writes up to `cap`
 * kernel durations [ms] to kernel_ms (host memory), returning how many were written. */
int adrp_profile_begin(adrp_t* h, int max_launches);
int adrp_profile_end(adrp_t* h, float* kernel_ms, int cap);

/* ---------------------------------------------------------------------------------------
 * Persistent step (HoverAviary, RPM / ONE_D_RPM actions, E <= 1024): BASELINE config 1, the
 * reference's one-env loop (examples/pid.py:101-147 calling BaseAviary.step, envs/BaseAviary.py:
 * 262-387) with no kernel launch per step.  begin launches one resident kernel (a workgroup per 64
 * envs) on its own stream and returns HOST pointers into a host-mapped mailbox: act [E][A] float,
 * obs [E][D] float, reward [E] float, terminated / truncated [E] uint8, terminal obs [E][D] float
 * (auto-reset envs).  step: the caller writes act, calls adrp_persistent_step, which returns when
 * the env.step is done and the outputs are in the mailbox (same results as adrp_step on the same
 * state).  While active, adrp_step / adrp_reset / adrp_get_state / adrp_set_state are refused.
 * end stops the kernel (destroy ends it too); the kernel also ends by itself after 10 s without a
 * request, after which step fails and end + begin restart it. */
int adrp_persistent_begin(adrp_t* h, void** act, void** obs, void** reward, void** terminated, void** truncated,
                          void** terminal_obs);
int adrp_persistent_step(adrp_t* h);
int adrp_persistent_end(adrp_t* h);

/* Diagnostics (off by default, costs a same-address atomic per touching wave):
 * count env-steps whose sub-steps touched the plane contact model. */
int adrp_set_diagnostics(adrp_t* h, int enable);
int adrp_diagnostic_contact_count(adrp_t* h, int reset);
/* Race handles: with diagnostics on, each env.step also records per drone a hash of the int16
 * (roll, pitch, yaw) moments of every firmware controllerMellinger call of the step, in call order
 * (FNV-1a over the int32 values, seed 2166136261, prime 16777619; oracle/race.c computes the same).
 * Parity tests use it as the causal witness of an int16 truncation difference.  Copies E * N values
 * of the last step to `out` (host memory); n must be E * N.  Replaces nothing in the reference. */
int adrp_race_moment_hash(adrp_t* h, uint32_t* out, size_t n);
/* Race handles, diagnostics level 2 (adrp_set_diagnostics(h, 2); the step then runs the one-lane
 * kernel): each env.step also records per drone the int16 (roll, pitch, yaw) of every firmware
 * controllerMellinger call, in call order (MellingerControl.py:413-415: control_t's moments).
 * Copies them to `out` [E*N][max_calls][3] and the number of calls to `counts` [E*N] (host memory);
 * n must be E * N and max_calls the sub-steps per env.step.  The oracle replays them
 * (oracle/race.c orc_race_set_moment_replay) to show that a drone whose truncation differs agrees
 * once the same integers are used.  Replaces nothing in the reference. */
int adrp_race_moment_log(adrp_t* h, int16_t* out, int32_t* counts, size_t n, int max_calls);
/* Race handles, diagnostics on: auto-resets of the four-lane kernel since the last read, out[0]
 * copied from a next-reset image (computed ahead by the refill launch every ADRP_RESET_IMAGES
 * steps, default 32, 0 = off), out[1] computed inline.  Replaces nothing in the reference. */
int adrp_race_reset_counts(adrp_t* h, int32_t* out, int reset);

/* ---------------------------------------------------------------------------------------
 * On-device policy forward: the actor of an SB3 PPO MlpPolicy
 * (in_dim -> hidden1 -> hidden2 -> 4, Tanh or ReLU) + the RLController action transform,
 * on f32 MFMA.  Replaces, batched, RLController.predict / _action_transform
 * (user_controller/RLController.py:39-73, RLControllerTwoGates.py:38-69) over
 * PPO.predict(obs, deterministic=True) (stable_baselines3 2.3.2: mlp_extractor.policy_net,
 * action_net, clip to the [-1, 1] Box).  Weights are host float32 arrays in torch Linear
 * layout ([out][in] row-major): the policy.pth tensors mlp_extractor.policy_net.{0,2}.* and
 * action_net.*.  obs rows are the first in_dim floats of each obs_stride-wide row (e.g.
 * adrp_step's obs_dev with rows = E*N); act_dev receives float [rows][4] (RELATIVE / ABSOLUTE,
 * and RAW with 4 actions) or [rows][act_dim] (RAW).  Policies with in_dim <= 64 and act_dim <= 4
 * run the narrow kernels; wider ones (in_dim <= 576 = ADRP_MAX_DRONES x 72, the joint
 * MultiHoverAviary row SB3's MlpPolicy flattens; act_dim <= 32) the wide kernels, as does every
 * policy created with ADRP_POLICY_WIDE=1 in the environment (csrc/policy_kernel.h).
 * --------------------------------------------------------------------------------------- */
#define ADRP_POLICY_TANH 0          /* SB3 MlpPolicy default activation_fn (nn.Tanh) */
#define ADRP_POLICY_RELU 1          /* policy_kwargs activation_fn=nn.ReLU (twogates.zip) */
#define ADRP_POLICY_RAW 0           /* act = clip(mean, -1, 1) */
#define ADRP_POLICY_RELATIVE 1      /* RLController: a[3]=0; obs[[0,1,2,5]] + a*[1,1,1,pi], yaw map2pi */
#define ADRP_POLICY_ABSOLUTE 2      /* RLControllerTwoGates: a[3]=0; a*[1,1,1,pi], yaw map2pi */

typedef struct adrp_policy adrp_policy_t;

/* hidden1, hidden2 in {16, 32, 64, 128}; in_dim 1..576; 4 actions */
int adrp_policy_create(int device, int in_dim, int hidden1, int hidden2, int activation,
                       const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* w3, const float* b3, adrp_policy_t** out);
int adrp_policy_act(adrp_policy_t* p, const float* obs_dev, int rows, int obs_stride, int mode,
                    float* act_dev, void* stream);
void adrp_policy_destroy(adrp_policy_t* p);
/* act_dim 1..32: the action_net's outputs (HoverAviary ONE_D_RPM 1, RPM 4; a joint MultiHoverAviary
 * agent N x A, row-major [drone][action] as SB3 reshapes the flat action).  RELATIVE / ABSOLUTE need
 * act_dim == 4; RAW takes any, in adrp_policy_act and adrp_policy_sample alike. */
int adrp_policy_create2(int device, int in_dim, int hidden1, int hidden2, int act_dim, int activation,
                        const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, adrp_policy_t** out);

/* The fragment blob a policy of this shape is uploaded as (host only, no device needed): returns its
 * size in floats or a negative ADRP_ERR_*; writes it to blob_out when blob_cap (floats) suffices, and
 * the layout (csrc/policy_kernel.h PolicyLayout, fields in declaration order: in_dim, f1, f2, f3, b1,
 * b2, b3, total, s1, t3, n_out, wide; the rest 0) to layout_out unless NULL.  wide != 0: the wide
 * kernels' layout even inside the narrow box (what ADRP_POLICY_WIDE=1 uploads); 0: what
 * adrp_policy_create2 picks.  Lane l of fragment (t, s) of layer 1 holds W1[16 t + (l & 15)][4 s + (l >> 4)],
 * of fragment (u, t, i) of layer 2 W2[16 u + (l & 15)][16 t + 4 (l >> 4) + i], of fragment (u3, u, i) of
 * layer 3 W3[16 u3 + (l & 15)][16 u + 4 (l >> 4) + i]; zeros beyond in_dim / n_out. */
int adrp_policy_fragments(int in_dim, int hidden1, int hidden2, int n_out, const float* w1, const float* b1,
                          const float* w2, const float* b2, const float* w3, const float* b3, int wide,
                          float* blob_out, int blob_cap, int layout_out[16]);

/* ---------------------------------------------------------------------------------------
 * On-device PPO rollout step (examples/learn.py:72-94 trains PPO): what SB3's
 * OnPolicyAlgorithm.collect_rollouts does per step, `actions, values, log_probs = policy(obs)`
 * with ActorCriticPolicy.forward(obs, deterministic=False) (stable_baselines3 2.3.2): the actor
 * mean (as adrp_policy_act), the critic mlp_extractor.value_net (in_dim -> hidden1 -> hidden2, the
 * same activation) + value_net (-> 1), a DiagGaussianDistribution sample a = mean +
 * exp(log_std) eps and log_prob = sum_i Normal(mean_i, std_i).log_prob(a_i).  eps ~ N(0, 1): one
 * Philox4x32-10 block per (row, output quad q), counter {row, counter, 0x504f4c00, q} keyed by seed,
 * Box-Muller of its word pairs (the race action noise's IEEE float form) for outputs 4q .. 4q+3;
 * log_prob is the float32 sum in ascending output index.  Replaces, batched on the device,
 * policy(obs_tensor) inside collect_rollouts plus the np.clip of the actions it sends the env.
 * adrp_policy_set_critic: value_net.{0,2}.* / value_net.* in torch layout and log_std [act_dim].
 * adrp_policy_sample: action_dev [rows][act_dim] (the sample, what the rollout buffer stores),
 * env_act_dev (clip to [-1, 1], then the mode transform; [rows][act_dim], RELATIVE / ABSOLUTE
 * [rows][4]), value_dev [rows], logprob_dev [rows], eps_dev [rows][act_dim] or NULL.
 * --------------------------------------------------------------------------------------- */
int adrp_policy_set_critic(adrp_policy_t* p, const float* vw1, const float* vb1, const float* vw2,
                           const float* vb2, const float* vw3, const float* vb3, const float* log_std);
int adrp_policy_sample(adrp_policy_t* p, const float* obs_dev, int rows, int obs_stride, int mode,
                       uint64_t seed, uint32_t counter, float* env_act_dev, float* action_dev,
                       float* value_dev, float* logprob_dev, float* eps_dev, void* stream);

/* GAE over a rollout (SB3 RolloutBuffer.compute_returns_and_advantage, stable_baselines3 2.3.2):
 * rewards / values / episode_starts [n_steps][n_envs] float32 on the device, last_values /
 * dones [n_envs]; writes advantages and returns [n_steps][n_envs] (returns = advantages + values).
 * One lane per env runs the backward recursion. */
int adrp_gae(const float* rewards, const float* values, const float* episode_starts, const float* last_values,
             const float* dones, int n_steps, int n_envs, double gamma, double gae_lambda, float* advantages,
             float* returns, void* stream);

/* ---------------------------------------------------------------------------------------
 * On-device PPO update (examples/learn.py:72-94: model.learn -> PPO.train): the clipped-surrogate
 * minibatch update of stable_baselines3 2.3.2 PPO.train() for the MlpPolicy above, restated from
 * SB3's published code (not pinned against an SB3 run): evaluate_actions at the stored, unclipped
 * actions, advantage normalisation (unbiased std, + 1e-8, n > 1), policy / value / entropy loss,
 * the gradient with respect to the 13 tensors (mlp_extractor.policy_net.{0,2}, action_net,
 * mlp_extractor.value_net.{0,2}, value_net, log_std), clip_grad_norm_ over all of them and
 * torch.optim.Adam (betas 0.9 / 0.999, eps 1e-5, no weight decay).  csrc/ppo_kernel.h.
 *
 * A learner is attached to a policy with a critic and takes its initial parameters from the
 * policy's device blobs.  Every update rewrites the policy's actor blob, critic blob and log_std in
 * place (the pointers never change: adrp_policy_act / adrp_policy_sample launched afterwards on
 * the same stream see the new weights, a captured graph stays valid).  Lifetime: destroy the learner
 * before its policy, and do not call adrp_policy_set_critic on a policy that has a learner.
 *
 * adrp_ppo_update: one minibatch of n rows idx[0..n) (int64, device) of the flattened rollout buffers
 * obs [rows][obs_stride], actions [rows][act_dim], old_values / old_log_prob / advantages / returns
 * [rows] (float32, device).  Four launches on `stream` (three without advantage normalisation), no host
 * synchronisation, capturable; Adam's step count lives on the device.  stats_out (device, 5 floats or NULL): policy_loss, value_loss,
 * entropy_loss, approx_kl, clip_fraction.  Results are bitwise reproducible.
 *
 * The flat parameter vector: the 13 tensors in the order above (actor 6, critic 6, log_std), each in
 * torch layout, adrp_ppo_param_count floats.  adrp_ppo_params copies parameters, Adam's m and v
 * (device, that many floats each) and t (device, one int32) out, any of them NULL to skip;
 * adrp_ppo_set_params copies them in (t < 0 keeps the step count) and re-packs the policy;
 * adrp_ppo_gradients copies the last update's raw (pre-clip) gradient out.
 * --------------------------------------------------------------------------------------- */
typedef struct adrp_ppo adrp_ppo_t;
typedef struct adrp_ppo_cfg {
    uint32_t struct_size;        /* sizeof(adrp_ppo_cfg) */
    int32_t normalize_advantage;
    double learning_rate;        /* > 0 */
    double clip_range;           /* >= 0 */
    double clip_range_vf;        /* < 0: none (SB3's default None) */
    double ent_coef;
    double vf_coef;
    double max_grad_norm;
} adrp_ppo_cfg;
int adrp_ppo_default_cfg(adrp_ppo_cfg* cfg);      /* SB3's defaults: 3e-4, 0.2, none, 0.0, 0.5, 0.5, normalise */
int adrp_ppo_create(adrp_policy_t* policy, const adrp_ppo_cfg* cfg, adrp_ppo_t** out);
int adrp_ppo_update(adrp_ppo_t* ppo, const float* obs, int obs_stride, const float* actions, const float* old_values,
                    const float* old_log_prob, const float* advantages, const float* returns, const int64_t* idx,
                    int n, float* stats_out, void* stream);
int adrp_ppo_param_count(const adrp_ppo_t* ppo);
int adrp_ppo_params(adrp_ppo_t* ppo, float* params_out, float* m_out, float* v_out, int32_t* t_out, void* stream);
int adrp_ppo_set_params(adrp_ppo_t* ppo, const float* params, const float* m, const float* v, int t, void* stream);
int adrp_ppo_gradients(adrp_ppo_t* ppo, float* grad_out, void* stream);
void adrp_ppo_destroy(adrp_ppo_t* ppo);

/* ---------------------------------------------------------------------------------------
 * On-device episode statistics (examples/learn.py:82-94, 142; scripts/sim.py:62-108): the episode
 * accounts stable_baselines3 2.3.2 keeps on the host, restated from its published code (not pinned
 * against an SB3 run): evaluation.py evaluate_policy's per-step `for i in range(n_envs)` loop
 * (current_rewards / current_lengths, episode_counts < episode_count_targets, the episode_rewards /
 * episode_lengths lists) and the Monitor window behind rollout/ep_rew_mean / ep_len_mean
 * (on_policy_algorithm.py ep_info_buffer = deque(maxlen=stats_window_size), utils.safe_mean).
 * Handle-less: the caller owns every buffer (all on one device) and passes them in one struct; every
 * pointer is fixed per step, so a step can be captured in a HIP graph.  csrc/episode.hip.
 *
 * adrp_episode_step: one launch (one workgroup) per env.step on the step's rew [E] float32 and
 * term / trunc [E] uint8.  Per env: run_return += (double)rew, run_length += 1.  Env e finishes when
 * term | trunc and is logged when quota is NULL or count[e] < quota[e].  The logged finishers of a step
 * are ranked by ascending env index (the order SB3's loop appends in); rank r goes to position
 * total + r (total = meta[0] before the step).  ring == 0: slot = position while it is < capacity,
 * otherwise the episode is only counted (meta[3]).  ring == 1: slot = position mod capacity, and of a
 * step with k > capacity logged finishers only ranks >= k - capacity are written (one writer per slot):
 * the log holds what deque(maxlen=capacity) holds.  A logged env gets count[e] += 1 and its run_return /
 * run_length go back to 0; those of an env past its quota are unspecified.  meta[0] += k, meta[2] += 1,
 * meta[1] is recomputed.  No atomics: equal inputs give equal bits.
 *
 * adrp_episode_summary: out8 (device, 8 doubles) = {n, mean return, std return (ddof 0, np.std), min
 * return, max return, mean length, std length, total} over the n = min(total, capacity) logged
 * episodes; double arithmetic in a fixed order, two-pass variance; n = 0 gives NaN (safe_mean).
 *
 * Errors are reported through adrp_last_error(NULL).  Refused with ADRP_ERR_INVALID before any device
 * call: NULL io, a struct_size mismatch, num_envs < 1, capacity < 1, ring not 0 / 1, a NULL buffer other
 * than quota, NULL rew / term / trunc / out8.
 * --------------------------------------------------------------------------------------- */
typedef struct adrp_episode_io {
    uint32_t struct_size;     /* sizeof(adrp_episode_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  capacity;        /* C >= 1 log slots */
    int32_t  ring;            /* 0: log the first C episodes (evaluation); 1: keep the last C (Monitor window) */
    const int32_t* quota;     /* int32 [E] or NULL: env e is logged only while count[e] < quota[e] */
    double*  run_return;      /* [E] running sum of the current episode (float64, as SB3's current_rewards) */
    int32_t* run_length;      /* [E] */
    int32_t* count;           /* [E] episodes logged for env e */
    int64_t* meta;            /* [4]: total episodes logged, remaining = sum_e max(0, quota[e] - count[e])
                                 (0 without quota), steps taken, episodes dropped (ring == 0 and the log is full) */
    double*  log_return;      /* [C] */
    int32_t* log_length;      /* [C] */
    int32_t* log_env;         /* [C] */
} adrp_episode_io;
int adrp_episode_step(const adrp_episode_io* io, const float* rew, const uint8_t* term, const uint8_t* trunc, void* stream);
int adrp_episode_summary(const adrp_episode_io* io, double* out8, void* stream);

/* ---------------------------------------------------------------------------------------
 * Batched race evaluation (scripts/sim.py:18-112 simulate(): one controller per drone, n_runs episodes, the
 * episode times): the two per-step pieces of that loop that are not the env step.  csrc/sim_kernel.h,
 * gym_pybullet_adrp_amd/sim.py.  Handle-less like the episode statistics: the caller owns every buffer (all
 * on one device), every pointer is fixed per step, so a wave's step sequence can be captured in a HIP graph.
 *
 * adrp_race_controllers: one launch per step, one lane per (env, drone), slot e * N + n.  Writes the command
 * arrays adrp_race_command takes, codes int32 [E,N] and args float64 [E,N,ADRP_CMD_ARGS], every slot on every
 * step (zeros included).  kind[n] picks drone n's controller:
 *   NONE       code ADRP_CMD_NONE, zeros.
 *   HARDCODED  user_controller/HardCodedController.py:117-190 as hardcoded.HardCodedCommander.predict restates
 *              it, bit for bit: step = clamp(trunc(ep_time * 25) - offset, 0, ref_len); TAKEOFF [0.3, 2] before
 *              take-off; FULLSTATE (ref[step], 0, 0.5, 0, 0, ep_time) while step < ref_len; then one NOTIFY
 *              [ep_time], one LAND [0, 2], then NONE.  ref float64 [E,N,ref_len,3] (the spline samples), offset
 *              int64 [E,N] ((2 + delay) * 25), phase uint8 [3][E*N] (took off, notified, landed), which the
 *              kernel updates.
 *   POLICY     RLController._action_transform (RLController.py:62-73): FULLSTATE with args[0:3] = the setpoint's
 *              x, y, z, args[9] = its yaw, args[13] = ep_time, the rest 0.  setpoints float32 [N][E][4],
 *              drone-major: what adrp_policy_act of drone n's policy writes from the rows obs_dev + n * D with
 *              rows = E and obs_stride = N * D, before this launch on the same stream.
 *
 * adrp_race_results_*: the per-drone twin of adrp_episode_step for envs without auto-reset, run in waves of
 * E episodes.  adrp_race_results_begin(io, base, n_open) opens a wave: running arrays to zero, finish / elim
 * to -1, open[e] = e < n_open, meta[1] = n_open, and io->base = base (a host field that travels with every
 * later step launch).  adrp_race_results_step: one launch (one workgroup) per env.step, after it, on the
 * step's rew [E] float32, term / trunc [E] uint8 and the per-drone gate / flags int32 [E*N] of the race state
 * (adrp_state_field "gate" / "flags": bit 0 eliminated, bit 1 finished).  For each env with open[e] != 0:
 * run_return += (double)rew, run_length += 1; per drone gates = gate, finish = run_length the first time
 * flags & 2, elim = run_length the first time flags & 1 (a drone may have both).  On term | trunc the episode
 * goes to log slot base + e (one writer per slot) and open[e] = 0: later steps change nothing of it.
 * meta[0] += episodes closed, meta[1] = envs still open (a fixed-order count, no atomic), meta[2] += 1.
 * adrp_race_results_step_env reads gate / flags from handle h's own device image in place.
 *
 * Errors are reported through adrp_last_error(NULL).  Refused with ADRP_ERR_INVALID before any device call:
 * a NULL io, a struct_size mismatch, num_envs < 1, num_drones outside 1..ADRP_MAX_DRONES, capacity < 1,
 * base < 0 or base + n_open > capacity, n_open outside 0..num_envs, a kind outside the three, a NULL required
 * buffer, HARDCODED without ref / offset / phase (or ref_len < 1), POLICY without setpoints, NULL gate / flags /
 * rew / term / trunc, a NULL or non-race handle, a handle whose E, N differ from the io's.
 * --------------------------------------------------------------------------------------- */
#define ADRP_RACE_CTRL_NONE 0
#define ADRP_RACE_CTRL_HARDCODED 1
#define ADRP_RACE_CTRL_POLICY 2
typedef struct adrp_race_ctrl_io {
    uint32_t struct_size;     /* sizeof(adrp_race_ctrl_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  num_drones;      /* N in 1..ADRP_MAX_DRONES */
    int32_t  ref_len;         /* L: samples per reference trajectory (HARDCODED) */
    int32_t  kind[ADRP_MAX_DRONES];   /* ADRP_RACE_CTRL_* of drone n < N */
    const double*  ref;       /* [E][N][L][3] or NULL without a HARDCODED drone */
    const int64_t* offset;    /* [E][N], likewise */
    uint8_t* phase;           /* [3][E*N], likewise */
    const float* setpoints;   /* [N][E][4] or NULL without a POLICY drone */
    int32_t* codes;           /* [E][N] out */
    double*  args;            /* [E][N][ADRP_CMD_ARGS] out, 16-byte aligned */
} adrp_race_ctrl_io;
typedef struct adrp_race_results_io {
    uint32_t struct_size;     /* sizeof(adrp_race_results_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  num_drones;      /* N in 1..ADRP_MAX_DRONES */
    int32_t  capacity;        /* C >= 1 log slots */
    int32_t  base;            /* log slot of env 0 in the current wave (set by adrp_race_results_begin) */
    int32_t  reserved;
    uint8_t* open;            /* [E] the env's episode is still running */
    double*  run_return;      /* [E] */
    int32_t* run_length;      /* [E] */
    int32_t* gates;           /* [E][N] gates passed so far */
    int32_t* finish;          /* [E][N] step the drone finished at, -1 = not yet */
    int32_t* elim;            /* [E][N] step the drone was eliminated at, -1 = not yet */
    int64_t* meta;            /* [4]: episodes logged, envs still open, steps taken, unused */
    double*  log_return;      /* [C] */
    int32_t* log_length;      /* [C] */
    uint8_t* log_term;        /* [C] */
    uint8_t* log_trunc;       /* [C] */
    int32_t* log_gates;       /* [C][N] */
    int32_t* log_finish;      /* [C][N] */
    int32_t* log_elim;        /* [C][N] */
} adrp_race_results_io;
int adrp_race_controllers(const adrp_race_ctrl_io* io, double ep_time, void* stream);
int adrp_race_results_begin(adrp_race_results_io* io, int base, int n_open, void* stream);
int adrp_race_results_step(const adrp_race_results_io* io, const int32_t* gate, const int32_t* flags, const float* rew,
                           const uint8_t* term, const uint8_t* trunc, void* stream);
int adrp_race_results_step_env(const adrp_race_results_io* io, adrp_t* h, const float* rew, const uint8_t* term,
                               const uint8_t* trunc, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-drone PPO agents of a multi-drone race (rollout.MultiAgentRolloutCollector): the bookkeeping that makes
 * every drone of a MultiRaceAviary(autoreset = 0) its own agent, one small launch per env.step.  One lane per
 * agent slot j = e * N + n.  csrc/agents_kernel.h.  Handle-less like the episode statistics: the caller owns
 * every buffer (all on one device), every pointer is fixed per step.  No atomics: equal inputs give equal bits.
 *
 * adrp_race_agents_reset: for every slot of an env with mask[e] != 0 (mask uint8 [E]; NULL: every env),
 * utils/wrapper.py RewardWrapper.reset per drone from the drone's own observation row obs + j * D (float32):
 * wr_gate = (int)row[48], wr_target = row[12:15], wr_prev = row[0:3], alive = 1, run_return = 0, run_length = 0.
 *
 * adrp_race_agents_step: after env.step, on the step's obs rows, the per-drone gate / flags int32 [E*N] of the
 * race state (bit 0 eliminated, bit 1 finished), the env's term / trunc uint8 [E] and boot_value float32 [E*N]
 * (the critic's values of the post-step rows).  Per slot:
 *   was_alive = alive; done_now = (flags & 3) != 0; newly = was_alive && done_now; fin = (flags & 2) != 0.
 *   r = RewardWrapper._compute_reward (wrapper.py:121-186) of this drone, float64 arithmetic on the float32 row:
 *       gate > wr_gate % 4: wr_gate = gate, r_passed = 5, and wr_target = row[12 + 4 gate : 15 + 4 gate] when
 *       gate < 4 && gate < num_gates;  r_col = -1 when newly && !fin;  r_lap = 10 when newly && fin;
 *       r = (|target - prev|_xy - |target - row|_xy) + (|target - prev|_z - |target - row|_z) + r_passed + r_col
 *       + r_lap (L2 in xy, L1 in z);  wr_prev = row[0:3].  The reference's env-level terminated / task_completed
 *       are the drone's own "became done" / "finished": with N = 1 it is the fused wrapper's reward.
 *   boot = was_alive && !done_now && trunc[e] && !term[e] (the time-limit bootstrap of SB3's collect_rollouts).
 *   rewards[j]    = was_alive ? (float)(r + (boot ? gamma * boot_value[j] : 0)) : 0   (selects: a dead slot's
 *                   row and a stale boot_value never reach a reward, whatever they hold)
 *   valid[j]      = was_alive
 *   next_start[j] = done_now || term[e] || trunc[e] ? 1 : 0
 *   ep_return[j], ep_length[j] = run_return + r, run_length + 1 where newly || (was_alive && (term[e] | trunc[e])):
 *                   the agent episode that ends here, without the bootstrap; NaN, 0 elsewhere
 *   alive = was_alive && !done_now.  wr_gate / wr_target / wr_prev / run_return / run_length change only where
 *   was_alive: a dead slot keeps its state until its env's adrp_race_agents_reset.
 * adrp_race_agents_step_env reads gate / flags from handle h's own device image in place.
 *
 * Errors are reported through adrp_last_error(NULL).  Refused with ADRP_ERR_INVALID before any device call:
 * a NULL io, a struct_size mismatch, num_envs < 1, num_drones outside 1..ADRP_MAX_DRONES, obs_dim < 49,
 * num_gates outside 0..ADRP_MAX_GATES, num_envs * num_drones * obs_dim past 2^31 - 1, a NULL buffer of the io,
 * NULL obs / gate / flags / term / trunc / boot_value / rewards / valid / next_start / ep_return / ep_length,
 * a NULL or non-race handle, a handle whose E, N, D differ from the io's.
 * --------------------------------------------------------------------------------------- */
#define ADRP_AGENTS_OBS_MIN 49      /* floats of an observation row the agents kernels read from (gate id at 48) */
typedef struct adrp_race_agents_io {
    uint32_t struct_size;     /* sizeof(adrp_race_agents_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  num_drones;      /* N in 1..ADRP_MAX_DRONES */
    int32_t  obs_dim;         /* D >= ADRP_AGENTS_OBS_MIN floats per (env, drone) row */
    int32_t  num_gates;       /* 0..ADRP_MAX_GATES (adrp_track.num_gates) */
    int32_t  reserved;
    int32_t* wr_gate;         /* [E*N] RewardWrapper.current_gate_id */
    double*  wr_target;       /* [E*N][3] RewardWrapper.current_target */
    double*  wr_prev;         /* [E*N][3] RewardWrapper.previous_pos */
    uint8_t* alive;           /* [E*N] the agent's episode is running */
    double*  run_return;      /* [E*N] sum of the raw rewards of the running agent episode */
    int32_t* run_length;      /* [E*N] */
} adrp_race_agents_io;
int adrp_race_agents_reset(const adrp_race_agents_io* io, const float* obs, const uint8_t* mask, void* stream);
int adrp_race_agents_step(const adrp_race_agents_io* io, const float* obs, const int32_t* gate, const int32_t* flags,
                          const uint8_t* term, const uint8_t* trunc, const float* boot_value, double gamma,
                          float* rewards, uint8_t* valid, float* next_start, double* ep_return, int32_t* ep_length,
                          void* stream);
int adrp_race_agents_step_env(const adrp_race_agents_io* io, adrp_t* h, const float* obs, const uint8_t* term,
                              const uint8_t* trunc, const float* boot_value, double gamma, float* rewards,
                              uint8_t* valid, float* next_start, double* ep_return, int32_t* ep_length, void* stream);

/* ---------------------------------------------------------------------------------------
 * Race rosters for per-drone PPO rollouts (rollout.RosterRolloutCollector): some drones of every env are samples
 * of the policy being trained (LEARNER), the others race them as the scripted HardCodedController (HARDCODED), a
 * frozen policy (POLICY) or not at all (NONE).  Three small launches per env.step, one lane per slot, 256-lane
 * blocks, no LDS, no atomics.  csrc/roster_kernel.h.  Handle-less: the caller owns every buffer (all on one
 * device), every pointer is fixed per step.  L = num_learners; learner l is drone d(l), the drone n with
 * learner_index[n] = l; learner column c = l * E + e (drone-major, as setpoints).
 *
 * adrp_race_roster_act: before env.step.  adrp_race_controllers' launch with the episode time taken per env,
 * ep_time = (double)clock[e] / ctrl_freq (an IEEE float64 division), and one more role: LEARNER is POLICY's
 * transform (FULLSTATE, args[0:3] = x, y, z, args[9] = yaw, args[13] = ep_time) of learner_act[learner_index[n]][e],
 * the env_act adrp_policy_sample wrote for the L * E compact rows.  NONE, HARDCODED and POLICY are
 * adrp_race_controllers' kinds, bit for bit (one device function serves both kernels).  Every slot of codes and
 * args is written on every call; phase is updated for HARDCODED drones; clock is only read.
 *
 * adrp_race_roster_tick: after the caller's masked env.reset.  For an env with mask[e] != 0 (mask uint8 [E];
 * NULL: every env) clock[e] = 0 and the three phase flags of its N slots are cleared; for every other env
 * clock[e] += 1.  One lane per slot, the n = 0 lane owns the clock.
 *
 * adrp_race_roster_step: adrp_race_agents_step for the learner drones alone, one lane per learner column c.  It
 * reads and updates the agent state (agents: the [E*N] arrays of adrp_race_agents_io as they are, so
 * adrp_race_agents_reset serves unchanged), the obs row, gate and flags of slot j = e * N + d(l), reads term /
 * trunc of env e and boot_value[c] (float32 [L*E]: the critic on the compact post-step rows), and writes rewards,
 * valid, next_start, ep_return, ep_length at c of [L*E] outputs: what adrp_race_agents_step writes at j, bit for
 * bit (one device function serves both kernels).  The state of the other slots is not touched.
 * adrp_race_roster_step_env reads gate / flags from handle h's own device image in place.
 *
 * Errors are reported through adrp_last_error(NULL).  Refused with ADRP_ERR_INVALID before any device call: a
 * NULL io, a struct_size mismatch, num_envs < 1, num_drones outside 1..ADRP_MAX_DRONES, num_learners outside
 * 1..num_drones, a role outside the four, a learner_index that is not a bijection of the LEARNER drones onto
 * 0..L-1 or is >= 0 on another role, ctrl_freq <= 0 (act, tick), a NULL clock / phase / codes / args (act, tick),
 * HARDCODED without ref / offset / ref_len >= 1, POLICY without setpoints, LEARNER without learner_act (act);
 * for the step what adrp_race_agents_step refuses, an agents io whose num_envs / num_drones differ from the
 * roster's, a NULL or non-race handle, a handle whose E, N, D differ from the io's.
 * --------------------------------------------------------------------------------------- */
#define ADRP_ROSTER_NONE 0          /* = ADRP_RACE_CTRL_NONE */
#define ADRP_ROSTER_HARDCODED 1     /* = ADRP_RACE_CTRL_HARDCODED */
#define ADRP_ROSTER_POLICY 2        /* = ADRP_RACE_CTRL_POLICY: a frozen policy's setpoints */
#define ADRP_ROSTER_LEARNER 3       /* the policy being trained */
typedef struct adrp_race_roster_io {
    uint32_t struct_size;     /* sizeof(adrp_race_roster_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  num_drones;      /* N in 1..ADRP_MAX_DRONES */
    int32_t  num_learners;    /* L in 1..N */
    int32_t  ref_len;         /* samples per reference trajectory (HARDCODED) */
    int32_t  reserved;
    double   ctrl_freq;       /* env.steps per second of episode time, > 0 */
    int32_t  role[ADRP_MAX_DRONES];            /* ADRP_ROSTER_* of drone n < N */
    int32_t  learner_index[ADRP_MAX_DRONES];   /* l of a LEARNER drone, -1 otherwise */
    int32_t* clock;           /* [E] env.steps since the env's reset */
    uint8_t* phase;           /* [3][E*N] took off, notified, landed (adrp_race_ctrl_io.phase) */
    const double*  ref;       /* [E][N][ref_len][3] or NULL without a HARDCODED drone */
    const int64_t* offset;    /* [E][N], likewise */
    const float* setpoints;   /* [N][E][4] or NULL without a POLICY drone, 16-byte aligned */
    const float* learner_act; /* [L][E][4], 16-byte aligned */
    int32_t* codes;           /* [E][N] out */
    double*  args;            /* [E][N][ADRP_CMD_ARGS] out, 16-byte aligned */
} adrp_race_roster_io;
int adrp_race_roster_act(const adrp_race_roster_io* io, void* stream);
int adrp_race_roster_tick(const adrp_race_roster_io* io, const uint8_t* mask, void* stream);
int adrp_race_roster_step(const adrp_race_roster_io* io, const adrp_race_agents_io* agents, const float* obs,
                          const int32_t* gate, const int32_t* flags, const uint8_t* term, const uint8_t* trunc,
                          const float* boot_value, double gamma, float* rewards, uint8_t* valid, float* next_start,
                          double* ep_return, int32_t* ep_length, void* stream);
int adrp_race_roster_step_env(const adrp_race_roster_io* io, const adrp_race_agents_io* agents, adrp_t* h, const float* obs,
                              const uint8_t* term, const uint8_t* trunc, const float* boot_value, double gamma,
                              float* rewards, uint8_t* valid, float* next_start, double* ep_return, int32_t* ep_length,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * Device spline planner of the scripted racer (user_controller/HardCodedController.py:63-115: 16 waypoints
 * from the drone's start and the nominal gates, scipy splprep(s = 0.1), splev at L parameter values): what
 * hardcoded.plan computes per drone on the host, for every (env, drone) of a wave in one launch.
 * csrc/spline_plan.h (the fit, shared with the CPU program csrc/plan_host.cpp), csrc/plan_kernel.h.
 * Handle-less like the race evaluation above: the caller owns every buffer, all on one device.
 *
 * One lane per (env, drone), slot e * N + n, reads the start x, y from obs[0:2] and the four gates' x, y from
 * obs[12:28] of its observation row obs + slot * obs_stride (float32, widened to float64), fits in float64
 * (FITPACK's fpparc: k = 3, unit weights, tol 1e-3, maxit 20) and the workgroup writes the samples
 * ref[slot][j] = spline(samples[j]), j < L.  samples is the caller's table (np.linspace(0, 1, L)).  With a
 * mask only the envs with mask[e] != 0 are planned; nothing of the other envs is read or written.
 * status[slot]: bit 0 the fit did not end with FITPACK's ier = 0 (re-plan that drone on the host), bit 1 a
 * sample z >= 2.5 (the reference's ceiling check), bits 8..15 the knot count n, bits 16..23 the iterations
 * of the smoothing parameter.  Optional outputs: knots [E][N][20] (zero past n), n_knots [E][N], coef
 * [E][N][3][16] (zero past n - 4); phase uint8 [3][E*N] (adrp_race_ctrl_io.phase) of the planned slots is cleared.
 *
 * Refused with ADRP_ERR_INVALID before any device call, through adrp_last_error(NULL): a NULL io, a
 * struct_size mismatch, num_envs < 1, num_drones outside 1..ADRP_MAX_DRONES, ref_len < 2, obs_stride < 28,
 * a NULL obs / samples / ref / status.
 * --------------------------------------------------------------------------------------- */
#define ADRP_PLAN_KNOTS 20          /* knots a 16-point cubic fit can have (m + k + 1) */
#define ADRP_PLAN_COEF 16           /* coefficients per coordinate, at most */
#define ADRP_PLAN_OBS_MIN 28        /* floats of an observation row the planner reads from */
#define ADRP_PLAN_NOT_IER0 1        /* status bit 0 */
#define ADRP_PLAN_CEILING 2         /* status bit 1 */
typedef struct adrp_race_plan_io {
    uint32_t struct_size;     /* sizeof(adrp_race_plan_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  num_drones;      /* N in 1..ADRP_MAX_DRONES */
    int32_t  ref_len;         /* L >= 2 samples per trajectory */
    int32_t  obs_stride;      /* floats between consecutive (env, drone) rows, >= 28 */
    int32_t  reserved;
    const float*   obs;       /* row e * N + n at obs + (e * N + n) * obs_stride */
    const uint8_t* mask;      /* [E] or NULL: every env */
    const double*  samples;   /* [L] */
    double*  ref;             /* [E][N][L][3] out */
    int32_t* status;          /* [E][N] out */
    double*  knots;           /* [E][N][ADRP_PLAN_KNOTS] out, or NULL */
    int32_t* n_knots;         /* [E][N] out, or NULL */
    double*  coef;            /* [E][N][3][ADRP_PLAN_COEF] out, or NULL */
    uint8_t* phase;           /* [3][E*N] cleared for the planned slots, or NULL */
} adrp_race_plan_io;
int adrp_race_plan(const adrp_race_plan_io* io, void* stream);

/* ---------------------------------------------------------------------------------------
 * Drone camera of the race scene (BaseAviary._getDroneImages, BaseAviary.py:569-621; the RGB observation of
 * MultiRaceAviary, MultiRaceAviary.py:300-304, 574-588): depth, segmentation and colour images of every
 * (env, drone) in one launch, by ray casting against the scene's analytic shapes: the ground plane, the
 * gates' and obstacles' URDF boxes and cylinders at the env's poses, the env's other drones as their
 * collision cylinders.  csrc/camera_core.h (view, part table, ray tests; shared with the CPU program
 * csrc/camera_host.cpp), csrc/camera_kernel.h.  Handle-less like the planner above: the caller owns every
 * buffer, all on one device.  DESIGN.md §3.19 states the camera model and its deviations from pybullet.
 *
 * View of drone slot e * N + n: eye = pos + (0, 0, L), L = 0.0397; forward f along R(quat) (1000, 0, 0) + pos -
 * eye, up = world z; 60 degrees vertical field of view, aspect 1, near = L, far = 1000.  Pixel (row i from the
 * top, column j) casts d = f + x s + y u, x = (2 (j + .5) / W - 1) tan 30, y = (1 - 2 (i + .5) / H) tan 30; the
 * nearest entry with near <= t <= far wins (t is the eye-space depth).
 * Outputs, each optional, contiguous [E][N][H][W]:
 *   dep float32: far / (far - near) (1 - near / t); 1 where nothing is hit
 *   seg int32:   body id + ((link + 1) << 24); plane 0, drone n -> 1 + n, gate g -> 1 + N + g, obstacle o ->
 *                1 + N + G + o; gate links: bottom bar 0, top 1, +x 2, -x 3, support 4; obstacle: cylinder -1,
 *                box 0; plane and drones -1; -1 where nothing is hit
 *   rgb uint8 [E][N][H][W][4]: the hit link's URDF material colour, alpha 255, unlit; 0 0 0 0 where nothing is hit
 * State planes as adrp_get_state lays them out, column e * N + n of E * N, float (precision 0) or double (1):
 * pos [3] (pos_x..z), quat [4] (quat_x..w), gates [16] (gate_g_x, _y, _z, _yaw), obstacles [12] (obst_o_x, _y, _z).
 * capture_freq > 0: only the (env, drone) with step_counter[e * N + n] % capture_freq == 0 are rendered
 * (BaseAviary.step's IMG_CAPTURE_FREQ test), the other images stay as they are; 0 renders all.  With a
 * mask only the envs with mask[e] != 0 are rendered.
 *
 * adrp_race_camera_env reads the state planes, the step counters and the track (num_gates, num_obstacles,
 * gate types) of a race handle instead of the io's (its state pointers and scene fields are ignored).
 *
 * Refused with ADRP_ERR_INVALID before any device call, through adrp_last_error(NULL): a NULL io, a
 * struct_size mismatch, num_envs < 1, num_drones outside 1..ADRP_MAX_DRONES, width or height < 1,
 * num_envs * num_drones at 2^24 or more (one workgroup each), num_envs * num_drones * height * width past
 * 2^31 - 1, no output pointer, an output pointer not 4-byte aligned, a negative capture_freq;
 * handle-less: num_gates / num_obstacles outside 0..4, precision not 0 / 1, a NULL pos / quat (gates /
 * obstacles when their count is not 0), capture_freq > 0 without step_counter; _env: a NULL handle, a handle
 * in persistent mode, a non-race handle, a handle of another E or N.
 * --------------------------------------------------------------------------------------- */
typedef struct adrp_race_camera_io {
    uint32_t struct_size;     /* sizeof(adrp_race_camera_io); checked */
    int32_t  num_envs;        /* E >= 1 */
    int32_t  num_drones;      /* N in 1..ADRP_MAX_DRONES */
    int32_t  width;           /* W >= 1 */
    int32_t  height;          /* H >= 1 */
    int32_t  num_gates;       /* 0..ADRP_MAX_GATES */
    int32_t  num_obstacles;   /* 0..ADRP_MAX_OBSTACLES */
    int32_t  gate_low[4];     /* gate g is a low portal (adrp_track.gates[g][6] > 0) */
    int32_t  precision;       /* of the state planes: 0 float, 1 double */
    int32_t  capture_freq;    /* 0: always */
    int32_t  reserved;
    const void* pos;          /* [3][E*N] */
    const void* quat;         /* [4][E*N] */
    const void* gates;        /* [16][E*N] */
    const void* obstacles;    /* [12][E*N] */
    const int32_t* step_counter;   /* [E*N], or NULL with capture_freq 0 */
    const uint8_t* mask;      /* [E] or NULL: every env */
    float*   dep;             /* [E][N][H][W] out, or NULL */
    int32_t* seg;             /* [E][N][H][W] out, or NULL */
    uint8_t* rgb;             /* [E][N][H][W][4] out, 4-byte aligned, or NULL */
} adrp_race_camera_io;
int adrp_race_camera(const adrp_race_camera_io* io, void* stream);
int adrp_race_camera_env(const adrp_race_camera_io* io, adrp_t* h, void* stream);

/* ---------------------------------------------------------------------------------------
 * Stand-alone batched DSLPIDControl (control/DSLPIDControl.py:9-259, control/BaseControl.py:21-95):
 * what examples/pid.py:126-147 and examples/downwash.py build one object per drone of, for users who
 * drive CtrlAviary themselves.  One controller handle holds `rows` independent controllers (one per
 * (env, drone) pair, rows = E * N, row e * N + n), their state SoA [9][rows] on the device in the
 * controller's precision: last_rpy 3, integral_pos_e 3, integral_rpy_e 3.  One kernel launch per
 * compute call on the caller's stream, no allocation and no host synchronisation (capturable); the
 * gains, the mixer and control_timestep travel by value with the launch, so a captured graph keeps the
 * values it was captured with.  csrc/dslpid_kernel.h.
 *
 * Errors of these calls are reported through adrp_last_error(NULL).  Argument errors (rows <= 0,
 * precision not 0 / 1, a struct_size mismatch, control_timestep <= 0, NULL pointers) are refused
 * before any device call.
 * --------------------------------------------------------------------------------------- */
#define ADRP_DSLPID_CF2X 0          /* MIXER_MATRIX of DroneModel.CF2X (DSLPIDControl.py:47-53) */
#define ADRP_DSLPID_CF2P 1          /* MIXER_MATRIX of DroneModel.CF2P (DSLPIDControl.py:54-60) */
typedef struct adrp_dslpid adrp_dslpid_t;
typedef struct adrp_dslpid_params {
    uint32_t struct_size;           /* = sizeof(adrp_dslpid_params); checked by create / set_gains */
    int32_t reserved;
    double p_for[3], i_for[3], d_for[3];   /* P / I / D_COEFF_FOR (setPIDCoefficients) */
    double p_tor[3], i_tor[3], d_tor[3];   /* P / I / D_COEFF_TOR */
    double mixer[4][3];             /* MIXER_MATRIX */
    double gravity;                 /* GRAVITY = g * m of the model's URDF (BaseControl.py:35) */
    double kf;                      /* KF (BaseControl.py:37) */
    double pwm2rpm_scale, pwm2rpm_const, min_pwm, max_pwm;   /* DSLPIDControl.py:43-46 */
} adrp_dslpid_params;
/* The reference's defaults (DSLPIDControl.py:37-60) for `model` (ADRP_DSLPID_CF2X / _CF2P), with
 * gravity = 9.8 * m and kf of the model's URDF (cf2x_IROS.urdf m = 0.03454, cf2p.urdf m = 0.027). */
int adrp_dslpid_default_params(int model, adrp_dslpid_params* p);
int adrp_dslpid_create(int rows, int precision, const adrp_dslpid_params* p, int device, adrp_dslpid_t** out);
void adrp_dslpid_destroy(adrp_dslpid_t* c);
/* DSLPIDControl.reset (:65-78): zero the nine state values of all rows (mask_dev NULL) or of the rows
 * with mask_dev[r] != 0 (uint8 [rows]).  control_counter is the caller's host-side count. */
int adrp_dslpid_reset(adrp_dslpid_t* c, const uint8_t* mask_dev, void* stream);
/* setPIDCoefficients: the six gain triples of *p replace the handle's (the other fields are ignored);
 * later compute calls use them. */
int adrp_dslpid_set_gains(adrp_dslpid_t* c, const adrp_dslpid_params* p);
/* [9][rows] in the controller's precision (float32 / float64) */
int adrp_dslpid_get_state(adrp_dslpid_t* c, void* st_dev, void* stream);
int adrp_dslpid_set_state(adrp_dslpid_t* c, const void* st_dev, void* stream);
/* computeControl of every row.  pos / quat (xyzw) / vel: component k of row r is base[r * row_stride + k];
 * row_stride 0 means three packed arrays [rows][3] / [rows][4] / [rows][3], and rows of
 * _getDroneStateVector's layout [rows][20] are passed as row, row + 3, row + 10 with row_stride 20.
 * input_precision is the element type of the three (0 float32, 1 float64): the controller's own, or
 * float32 into a float64 controller (converted on load); anything else is refused.  The targets are
 * [rows][3] in the controller's precision, NULL = zeros (of target_rpy only the yaw enters,
 * DSLPIDControl.py:200).  Outputs in the controller's precision: rpm_out [rows][4] (what adrp_step_rpm
 * takes), pos_e_out [rows][3] or NULL, yaw_e_out [rows] or NULL: computed_target_rpy[2] - cur_rpy[2]
 * (:145), the first the third angle of the intrinsic 'XYZ' decomposition of the target basis (:205). */
int adrp_dslpid_compute(adrp_dslpid_t* c, double control_timestep, const void* pos_dev, const void* quat_dev,
                        const void* vel_dev, int row_stride, int input_precision, const void* target_pos_dev,
                        const void* target_rpy_dev, const void* target_vel_dev, const void* target_rpy_rates_dev,
                        void* rpm_out, void* pos_e_out, void* yaw_e_out, void* stream);
/* The same with pos / quat / vel read from the state columns of env handle h (pos_*, quat_*, vel_* of
 * adrp_state_layout) in the handle's own precision: no float32 observation row in between, which is what
 * lets a float64 loop follow the reference to 1e-9.  Refused: a MultiRaceAviary handle, a handle whose
 * E * N or precision differs from the controller's, a handle in persistent mode. */
int adrp_dslpid_compute_env(adrp_dslpid_t* c, double control_timestep, adrp_t* h, const void* target_pos_dev,
                            const void* target_rpy_dev, const void* target_vel_dev, const void* target_rpy_rates_dev,
                            void* rpm_out, void* pos_e_out, void* yaw_e_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Stand-alone batched MellingerControl (control/MellingerControl.py:17-699): the Crazyflie firmware
 * controller that examples/cf.py / CFAviary step at 500 Hz, for users who drive CtrlAviary themselves.
 * One handle holds `rows` independent controllers (row e * N + n): the wrapper state and the firmware's
 * in the handle's precision, the high-level commander's as adrp_get_command_state describes it.  Every
 * call is one kernel launch on the caller's stream, without allocation or host synchronisation
 * (capturable).  The controller code is the race step kernels' (csrc/race_kernel.h mellinger_compute,
 * csrc/commander.h); csrc/mellinger_kernel.h only moves a row's state in and out.
 *
 * There is no command queue: adrp_mellinger_command processes its message at once, as the reference's
 * low_level_control does (send*Cmd, then process_command_queue(args[-1])).
 *
 * Errors of these calls are reported through adrp_last_error(NULL).  Argument errors (rows <= 0,
 * precision not 0 / 1, NULL pointers, a negative stride) are refused before any device call.
 * --------------------------------------------------------------------------------------- */
typedef struct adrp_mellinger adrp_mellinger_t;
int adrp_mellinger_create(int rows, int precision, int device, adrp_mellinger_t** out);
void adrp_mellinger_destroy(adrp_mellinger_t* c);
/* MellingerControl.reset(init_obs) (:99-150) of all rows (mask_dev NULL) or of the rows with
 * mask_dev[r] != 0 (uint8 [rows]): filters, integrators, histories, tick, last_*_tick, tumble and the
 * last controls / rpm cleared, prev_rpy / prev_vel from the given rows, the setpoint zeroed with the
 * override on, the commander idle and told the state (position, yaw; at rest).  pos / rpy / vel:
 * packed [rows][3] in the handle's precision.  Other rows are left alone. */
int adrp_mellinger_reset(adrp_mellinger_t* c, const void* pos_dev, const void* rpy_dev, const void* vel_dev,
                         const uint8_t* mask_dev, void* stream);
/* One command message per row, packed as for adrp_race_command: codes_dev int32 [rows] ADRP_CMD_*,
 * args_dev float64 [rows][ADRP_CMD_ARGS]; ADRP_CMD_NONE leaves a row untouched. */
int adrp_mellinger_command(adrp_mellinger_t* c, const int32_t* codes_dev, const double* args_dev, void* stream);
/* MellingerControl.computeControl (:154-262) of every row, once.  pos / rpy / vel: component k of row r is
 * base[r * row_stride + k]; row_stride 0 means three packed arrays [rows][3], and rows of
 * _getDroneStateVector's layout [rows][20] are passed as row, row + 7, row + 10 with row_stride 20.
 * input_precision is the element type of the three (0 float32, 1 float64): the handle's own, or float32
 * into a float64 handle (converted on load).  disturbance_dev: [rows][4] in the handle's precision, the
 * per-motor thrust disturbance the reference passes in the target_pos slot, NULL = zeros.  rpm_out:
 * [rows][4] in the handle's precision (what adrp_step_rpm takes). */
int adrp_mellinger_compute(adrp_mellinger_t* c, const void* pos_dev, const void* rpy_dev, const void* vel_dev,
                           int row_stride, int input_precision, const void* disturbance_dev, void* rpm_out,
                           void* stream);
/* The same with pos / vel read from the state columns of CtrlAviary handle h and roll / pitch / yaw taken
 * from its quaternion columns by the race kernels' Euler function; rpy_out ([rows][3], handle precision)
 * receives those angles, or is NULL.  Refused: a handle of another task, one whose E * N, precision or
 * device differs from the controller's. */
int adrp_mellinger_compute_env(adrp_mellinger_t* c, adrp_t* h, const void* disturbance_dev, void* rpm_out,
                               void* rpy_out, void* stream);
/* Controller state: nf float fields (handle precision) and ni int32 fields, each a contiguous [rows]
 * vector; the names are those of the race state's controller part (adrp_state_field of a race handle):
 * rpm_*, prev_rpm_*, prev_rpy_*, prev_vel_*, lpf_d1_*, lpf_d2_*, i_err_*, i_err_m_*, prev_omega_roll /
 * pitch, prev_sp_roll / pitch, ctl_roll / pitch / yaw / thrust (the int16 moments of the last firmware
 * call); tick, last_att_tick, last_pos_tick, tumble.  A negative tick counts as 0.  The layout is the
 * same for every handle: adrp_mellinger_state_layout takes NULL for c as well. */
int adrp_mellinger_state_layout(const adrp_mellinger_t* c, int* nf, int* ni);
const char* adrp_mellinger_state_field(int is_int, int index);
int adrp_mellinger_get_state(adrp_mellinger_t* c, void* f_dev, int32_t* i_dev, void* stream);
int adrp_mellinger_set_state(adrp_mellinger_t* c, const void* f_dev, const int32_t* i_dev, void* stream);
/* float [ADRP_CMD_NF][rows], int32 [ADRP_CMD_NI][rows], as adrp_get_command_state */
int adrp_mellinger_get_command_state(adrp_mellinger_t* c, float* f_dev, int32_t* i_dev, void* stream);
int adrp_mellinger_set_command_state(adrp_mellinger_t* c, const float* f_dev, const int32_t* i_dev, void* stream);

/* SB3 VecEnv host path: the terminal observations of the finished envs, compacted on the device
 * behind the step's packed outputs so ONE device -> host copy returns them (replaces the per-env
 * infos[e]["terminal_observation"] = obs that stable_baselines3 DummyVecEnv.step_wait fills from
 * its sub-envs, vec_env/dummy_vec_env.py, 2.3.2).  term / trunc [n] uint8, rows [n][row_floats]
 * (the env's terminal-obs buffer); writes count[0] = number of envs with term | trunc, idx[j] = the
 * j-th such env (ascending, j < count, so idx holds up to n entries) and out_rows[j] = rows[idx[j]]
 * for j < min(count, cap).  One workgroup; stream-ordered after the step. */
int adrp_compact_rows(const uint8_t* term, const uint8_t* trunc, const float* rows, int n, int row_floats,
                      int cap, int32_t* count, int32_t* idx, float* out_rows, void* stream);
/* The same host path's copies (kind 1: host -> device, 2: device -> host; pinned host memory makes
 * them asynchronous on the stream) and its one wait, without a framework dispatch in between. */
int adrp_memcpy_async(void* dst, const void* src, size_t bytes, int kind, void* stream);
int adrp_stream_synchronize(void* stream);

/* SB3 VecEnv host path in ONE call per step (vec_env.py AviaryVecEnv; replaces what
 * stable_baselines3 DummyVecEnv.step_async / step_wait do around the reference's env.step,
 * examples/learn.py:53-57, 72): the step kernel reads the actions from, and writes obs / reward
 * straight into, pinned host memory (device-mapped: no copy engine on the path), a compaction
 * writes the terminated / truncated / done flags, the finished envs' count and ids and their
 * terminal rows into the same host block, and the host waits once.  A handle holds
 * ADRP_VEC_SLOTS such host blocks (a ring: the caller's views of slot k stay valid until slot k is
 * stepped again); adrp_vec_bind records one (host pointers of hipHostMalloc'd / pinned memory,
 * translated to device addresses here), adrp_vec_step(h, k, stream) steps into it.  term_dev /
 * trunc_dev / tobs_dev / idx_dev are the caller's device buffers ([E] u8, [E] u8, [E][N][D] f32,
 * [E] i32): the step's own flags and terminal obs, the compaction's scratch.  Rows beyond cap are
 * left in tobs_dev (count says how many envs finished).  Stream-ordered; returns after the wait. */
#define ADRP_VEC_SLOTS 4
typedef struct adrp_vec_io {
    const float* act;            /* host [E][N][A] float32 (read by the step kernel) */
    float* obs;                  /* host [E][N][D] */
    float* rew;                  /* host [E] */
    uint8_t* term;               /* host [E] terminated */
    uint8_t* trunc;              /* host [E] truncated */
    uint8_t* done;               /* host [E] terminated | truncated */
    int32_t* count;              /* host [1] finished envs */
    int32_t* idx;                /* host [E] their ids, ascending */
    float* rows;                 /* host [cap][N*D] their terminal rows */
    int cap;
    uint8_t* term_dev;
    uint8_t* trunc_dev;
    float* tobs_dev;
    int32_t* idx_dev;
} adrp_vec_io;
int adrp_vec_bind(adrp_t* h, int slot, const adrp_vec_io* io);
int adrp_vec_step(adrp_t* h, int slot, void* stream);

/* ---------------------------------------------------------------------------------------
 * Parity mode noise (MultiRaceAviary).  The reference draws, per sub-step, the disturbance force
 * of every drone (np_random.<distrib>(low, high), MultiRaceAviary.py:532-537) and then the (N, 4)
 * action noise (np_random.<distrib>(0, std, (N, 4)), :223-228).  After adrp_set_noise the race
 * step takes them from these caller-owned DEVICE arrays instead of its Philox streams:
 *   act_noise_dev [E*N][S][4], force_dev [E*N][S][3] float64, drone slot e*N + n, sub-step s of
 *   the NEXT adrp_step (S = pyb_freq / ctrl_freq); the caller refills them (stream-ordered)
 *   before every step.  The pointers are kept until adrp_set_noise(h, NULL, NULL).  Only used when
 *   the track has disturbances on.  Replaces: nothing in the reference's API (its RNG is internal);
 *   lets a noisy reference step be replayed with the reference's own draws.
 * --------------------------------------------------------------------------------------- */
int adrp_set_noise(adrp_t* h, const double* act_noise_dev, const double* force_dev);

/* ---------------------------------------------------------------------------------------
 * Numerics probe (no reference counterpart: test support).  Evaluates one of the fp64
 * fast transcendentals the fp64 step kernels inline (csrc/adrp_device.h namespace f64:
 * refined v_rcp_f64 / v_rsq_f64, range-reduced polynomials) on n device doubles:
 * out[i] = f(in[i]); ATAN2 reads y = in[i], x = in[n + i], DIVC x = in[i], c = in[n + i].
 * Stream-ordered.
 * --------------------------------------------------------------------------------------- */
#define ADRP_MATH_RCP 0
#define ADRP_MATH_RSQ 1
#define ADRP_MATH_SQRT 2
#define ADRP_MATH_SIN_SMALL 3      /* |x| <= pi/8 */
#define ADRP_MATH_COS_SMALL 4      /* |x| <= pi/8 */
#define ADRP_MATH_ATAN2 5
#define ADRP_MATH_ASIN 6           /* |x| < 1 */
#define ADRP_MATH_EXP 7            /* x <= 0 in the kernels */
#define ADRP_MATH_SQRT_NN 8        /* sums of squares: x >= 0 or NaN (Bullet step norms) */
#define ADRP_MATH_RCP_NC 9         /* finite, non-zero x (no non-finite fix-up) */
#define ADRP_MATH_RSQ_NC 10        /* finite, positive x (quaternion norm) */
#define ADRP_MATH_SIN_TINY 11      /* |x| <= 0.03 (exp-map half angle) */
#define ADRP_MATH_COS_TINY 12      /* |x| <= 0.03 */
#define ADRP_MATH_EXPMAP_SINC 13   /* sin(x)/x of the hover exp map (per-lane series choice) */
#define ADRP_MATH_EXPMAP_COS 14    /* cos(x) of the hover exp map */
#define ADRP_MATH_QUAT_INV_NORM 15 /* 1/sqrt(n2) of the hover exp-map quaternion (per-lane form) */
#define ADRP_MATH_NORMAL_Z0 16     /* race action-noise Box-Muller of a Philox word pair: in[i]'s bits */
#define ADRP_MATH_NORMAL_Z1 17     /*   = x1 << 32 | x0; out = z0 / z1 (float samples, as doubles) */
#define ADRP_MATH_DIVC 18          /* in[i] / in[n + i] by the fp64 kernels' constant-divisor form */
#define ADRP_MATH_SIN_FAST 19      /* octant-reduced sin / cos (gate yaws, reset attitudes) */
#define ADRP_MATH_COS_FAST 20
#define ADRP_MATH_EXP_TAB 21       /* exp(x), x <= 0, table form of the fp64 race downwash */
#define ADRP_MATH_ATAN2_NC 22      /* atan2(in[i], in[n + i]) for finite operands (race Euler angles) */
#define ADRP_MATH_FDIV_RCP 23      /* float(in[i]) / float(in[n + i]) as the fp64 race firmware divides (f64::fdiv_rcp) */
int adrp_math_probe(int fn, const double* in_dev, double* out_dev, int n, void* stream);

/* The vector form: the attitude conversions and the fp32 fast forms of csrc/adrp_device.h, evaluated in
 * float (precision 0) or double (precision 1) on planes in_dev[k_in][n] -> out_dev[k_out][n] of device
 * doubles (a float evaluation rounds its inputs to float and widens its results).  Column i runs in lane
 * i % 64 of wave i / 64, so the caller decides which columns share a wave-uniform vote.  Quaternions are
 * xyzw, angles roll, pitch, yaw.  adrp_math_probe_v_planes reports k_in / k_out of a form. */
#define ADRP_MATHV_EULER_XYZ 0            /* q[4] -> rpy[3]: libm atan2 / asin (the DSLPID controller input) */
#define ADRP_MATHV_EULER_XYZ_FAST 1       /* q[4] -> rpy[3]: fatan2_ / fasin_, per-lane gimbal branches */
#define ADRP_MATHV_EULER_XYZ_FAST_U 2     /* q[4] -> rpy[3]: the same behind the wave-uniform gimbal vote */
#define ADRP_MATHV_QUAT_FROM_EULER 3      /* rpy[3] -> q[4]: libm sincos */
#define ADRP_MATHV_QUAT_FROM_EULER_FAST 4 /* rpy[3] -> q[4]: the small series when all half angles <= pi/8 */
#define ADRP_MATHV_FATAN2 5               /* (y, x) -> fatan2_(y, x) */
#define ADRP_MATHV_FASIN 6                /* s -> fasin_(s), |s| < 1 */
#define ADRP_MATHV_FEXP 7                 /* x -> fexp_(x), x <= 0 in the kernels */
#define ADRP_MATHV_SMALL_SINCOS 8         /* x -> (sin x, cos x), |x| <= pi/8 */
#define ADRP_MATHV_EXPMAP_SINC_COS 9      /* x -> (sin(x) / x, cos x), |x| <= pi/8 */
#define ADRP_MATHV_QUAT_INV_NORM 10       /* n2 -> 1 / sqrt(n2) */
#define ADRP_MATHV_CLAMP100_WV 11         /* (w[3], v[3]) -> the same clamped to [-100, 100] (clamp100_wv) */
int adrp_math_probe_v_planes(int fn, int* k_in, int* k_out);
int adrp_math_probe_v(int fn, int precision, const double* in_dev, double* out_dev, int n, void* stream);

/* the training-loop additions: the target_kl latch and rate setters of the PPO update, the learner-ended
 * reset mask of the race rosters */
#include "adrp_train.h"

#ifdef __cplusplus
}
#endif

#endif /* ADRP_H */
