// adrp.hip — libadrp.so: the C-ABI of include/adrp.h over the fused HIP kernels.
//
// Build (gfx950 only):  see gym_pybullet_adrp_amd/csrc/Makefile
// No CPU fallback: every entry point that computes needs a HIP device and fails with
// ADRP_ERR_DEVICE otherwise.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "adrp_internal.h"
#include "hover_persist.h"

static thread_local std::string g_err;

int seterr(adrp_t* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    g_err = msg;
    return code;
}

extern "C" int adrp_abi_version(void) { return ADRP_ABI_VERSION; }

extern "C" const char* adrp_last_error(const adrp_t* h) { return h ? h->err.c_str() : g_err.c_str(); }

// ---------------------------------------------------------------------------------------------
// defaults (reference constructors; cf2x_IROS.urdf constants; level0.yaml track)
// ---------------------------------------------------------------------------------------------
extern "C" int adrp_default_config(int task, adrp_config* c) {
    if (!c || (task != ADRP_TASK_HOVER && task != ADRP_TASK_RACE && task != ADRP_TASK_MULTIHOVER && !is_ctrl_task(task)))
        return seterr(nullptr, ADRP_ERR_INVALID, "task");
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(adrp_config);
    c->task = task;
    c->physics = ADRP_PHYS_PYB;
    c->num_envs = 1;
    c->autoreset = 1;
    c->link_frame_lag = 1;
    c->gravity = 9.8;                                        // BaseAviary.py:74
    adrp_drone_params& d = c->drone;                         // assets/cf2x_IROS.urdf
    d.m = 0.03454; d.l = 0.0397; d.thrust2weight = 2.25;
    d.ixx = 1.4e-5; d.iyy = 1.4e-5; d.izz = 2.17e-5;
    d.kf = 3.16e-10; d.km = 7.94e-12;
    d.collision_h = 0.025; d.collision_r = 0.06; d.collision_z_offset = 0.0;
    d.max_speed_kmh = 30.0; d.gnd_eff_coeff = 11.36859; d.prop_radius = 2.31348e-2;
    d.drag_coeff[0] = 9.1785e-7; d.drag_coeff[1] = 9.1785e-7; d.drag_coeff[2] = 10.311e-7;
    d.dw_coeff[0] = 2267.18; d.dw_coeff[1] = 0.16; d.dw_coeff[2] = -0.11;
    const double pp[4][2] = {{0.028, 0.028}, {-0.028, 0.028}, {-0.028, -0.028}, {0.028, -0.028}};
    for (int i = 0; i < 4; ++i) { d.prop_pos[i][0] = pp[i][0]; d.prop_pos[i][1] = pp[i][1]; }
    if (task == ADRP_TASK_HOVER || task == ADRP_TASK_MULTIHOVER || is_ctrl_task(task)) {
        c->act_type = ADRP_ACT_RPM;
        c->num_drones = 1;
        c->pyb_freq = 240; c->ctrl_freq = 30;                // HoverAviary.py:18-19
        c->action_buffer_size = 15;                          // ctrl_freq//2 (BaseRLAviary.py:66)
        c->init_xyz[0][2] = d.collision_h / 2 - d.collision_z_offset + 0.1;  // BaseAviary.py:195-197
        c->target_pos[2] = 1.0;
        c->episode_len_sec = 8.0;
        if (task == ADRP_TASK_MULTIHOVER) {                  // MultiHoverAviary.py:17 num_drones = 2
            c->num_drones = 2;
            for (int n = 0; n < c->num_drones; ++n) {        // BaseAviary.py:194-197
                c->init_xyz[n][0] = 4 * d.l * n; c->init_xyz[n][1] = 4 * d.l * n;
                c->init_xyz[n][2] = d.collision_h / 2 - d.collision_z_offset + 0.1;
            }
        }
        if (is_ctrl_task(task)) {                            // CtrlAviary.py:16-20, VelocityAviary.py:16-22
            c->act_type = task == ADRP_TASK_CTRL ? ADRP_ACT_RAW_RPM : ADRP_ACT_VEL;
            c->pyb_freq = 240; c->ctrl_freq = 240;
            // one drone; the rows of all eight are filled, so that raising num_drones alone gives the
            // reference's default formation (BaseAviary.py:194-197)
            for (int n = 0; n < ADRP_MAX_DRONES; ++n) {
                c->init_xyz[n][0] = 4 * d.l * n; c->init_xyz[n][1] = 4 * d.l * n;
                c->init_xyz[n][2] = d.collision_h / 2 - d.collision_z_offset + 0.1;
            }
        }
    } else {
        c->act_type = ADRP_ACT_FULLSTATE;
        c->num_drones = 2;
        c->pyb_freq = 500; c->ctrl_freq = 25;                // constants.py:29-31
        adrp_track& t = c->track;
        const double gates[4][7] = {{0.45, -1.0, 0.525, 0, 0, 2.35, 1}, {1.0, -1.55, 1.0, 0, 0, -0.78, 0},
                                    {0.0, 0.5, 0.525, 0, 0, 0, 1}, {-0.5, -0.5, 1.0, 0, 0, 3.14, 0}};
        const double obst[4][6] = {{1.0, -0.5, 0.525, 0, 0, 0}, {0.5, -1.5, 0.525, 0, 0, 0},
                                   {-0.5, 0, 0.525, 0, 0, 0}, {0, 1.0, 0.525, 0, 0, 0}};
        t.num_gates = 4; t.num_obstacles = 4;
        memcpy(t.gates, gates, sizeof gates);
        memcpy(t.obstacles, obst, sizeof obst);
        t.bounds_hi[0] = 3; t.bounds_hi[1] = 3; t.bounds_hi[2] = 2;
        t.episode_len_sec = 33;
        t.random_drone_state = 1;
        t.pos_offset_range[0][0] = -0.1; t.pos_offset_range[0][1] = 0.1;
        t.pos_offset_range[1][0] = -0.1; t.pos_offset_range[1][1] = 0.1;
        t.pos_offset_range[2][0] = 0.0;  t.pos_offset_range[2][1] = 0.02;
        for (int k = 0; k < 3; ++k) { t.rot_offset_range[k][0] = -0.1; t.rot_offset_range[k][1] = 0.1; }
        t.init_pos[0][0] = 0.9; t.init_pos[0][1] = 0.9; t.init_pos[0][2] = 0.05;
        t.init_pos[1][0] = 1.1; t.init_pos[1][1] = 1.1; t.init_pos[1][2] = 0.05;
        t.init_pos[2][0] = 0.7; t.init_pos[2][1] = 0.9; t.init_pos[2][2] = 0.05;   // N>2 extension
        t.init_pos[3][0] = 1.3; t.init_pos[3][1] = 1.1; t.init_pos[3][2] = 0.05;
        t.race_mass = 0.027;                                 // assets/cf2x.urdf:11
        t.race_inertia[0] = 1.4e-5; t.race_inertia[1] = 1.4e-5; t.race_inertia[2] = 2.17e-5;
    }
    return ADRP_OK;
}

static void derived(const adrp_config& c, double* hover_rpm, double* gnd_clip) {
    const adrp_drone_params& d = c.drone;
    const double gravity = c.gravity * d.m;
    *hover_rpm = sqrt(gravity / (4 * d.kf));
    const double maxr = sqrt((d.thrust2weight * gravity) / (4 * d.kf));
    const double maxt = 4 * d.kf * maxr * maxr;
    *gnd_clip = 0.25 * d.prop_radius * sqrt((15 * maxr * maxr * d.kf * d.gnd_eff_coeff) / maxt);
}

static int trunc_steps(double episode_len_sec, int pyb_freq) {
    // truncated when step_counter / PYB_FREQ > EPISODE_LEN_SEC in float64 (HoverAviary.py:114,
    // MultiRaceAviary.py:709): the smallest such step_counter
    long long t = (long long)floor(episode_len_sec * pyb_freq) - 2;
    if (t < 0) t = 0;
    while (!((double)t / (double)pyb_freq > episode_len_sec)) ++t;
    return (int)t;
}
static int trunc_steps(const adrp_config& c) { return trunc_steps(c.episode_len_sec, c.pyb_freq); }

template <typename Real>
static HoverConst<Real> hover_const(const adrp_config& c) {
    const adrp_drone_params& d = c.drone;
    HoverConst<Real> a;
    memset(&a, 0, sizeof a);
    a.S = c.pyb_freq / c.ctrl_freq;
    a.trunc_steps = trunc_steps(c);
    a.link_lag = c.link_frame_lag ? 1 : 0;
    a.physics = c.physics;
    a.dt = Real(1.0 / c.pyb_freq);
    a.mass = Real(d.m); a.inv_mass = Real(1.0 / d.m); a.gravity = Real(c.gravity);
    a.ixx = Real(d.ixx); a.iyy = Real(d.iyy); a.izz = Real(d.izz);
    a.inv_ixx = Real(1.0 / d.ixx); a.inv_iyy = Real(1.0 / d.iyy); a.inv_izz = Real(1.0 / d.izz);
    a.ang_max = Real(0.5 * (M_PI / 2) * c.pyb_freq);
    a.kf = Real(d.kf); a.km = Real(d.km);
    double hover_rpm, gnd_clip;
    derived(c, &hover_rpm, &gnd_clip);
    a.hover_rpm = Real(hover_rpm);
    for (int i = 0; i < 4; ++i) {
        a.px[i] = Real(d.prop_pos[i][0]); a.py[i] = Real(d.prop_pos[i][1]); a.pz[i] = Real(d.prop_pos[i][2]);
    }
    a.gnd_kf = Real(d.kf * d.gnd_eff_coeff);
    a.prop_r4 = Real(d.prop_radius / 4);
    a.gnd_clip = Real(gnd_clip);
    for (int k = 0; k < 3; ++k) a.drag[k] = Real(d.drag_coeff[k]);
    a.dyn_arm = Real(d.l / sqrt(2.0));
    a.coll_hh = Real(0.5 * d.collision_h); a.coll_r = Real(d.collision_r); a.coll_zoff = Real(d.collision_z_offset);
    for (int k = 0; k < 3; ++k) a.target[k] = Real(c.target_pos[k]);
    a.pid_grav = Real(c.gravity * d.m);
    a.pid_inv4kf = Real(1.0 / (4 * d.kf));
    a.ctrl_dt = Real(1.0 / c.ctrl_freq);
    a.ctrl_hz = Real(c.ctrl_freq);
    a.speed_limit = float(0.03 * d.max_speed_kmh * (1000.0 / 3600));   // BaseRLAviary.py:95
    return a;
}

template <typename Real>
static HoverReset<Real> hover_reset_dist(const adrp_config& c) {
    HoverReset<Real> r;
    memset(&r, 0, sizeof r);
    for (int k = 0; k < 3; ++k) {
        r.init_xyz[k] = Real(c.init_xyz[0][k]); r.init_rpy[k] = Real(c.init_rpy[0][k]);
        r.n_xyz[k] = Real(c.init_xyz_noise[k]); r.n_rpy[k] = Real(c.init_rpy_noise[k]);
        r.n_vel[k] = Real(c.init_vel_noise[k]); r.n_om[k] = Real(c.init_omega_noise[k]);
    }
    return r;
}

// the compiled-in constants are used only when the runtime block is bit-identical
template <typename Real>
static bool is_cf2x(const adrp_config& c) {
    const HoverConst<Real> rt = hover_const<Real>(c);
    HoverConst<Real> ct;
    memset(&ct, 0, sizeof ct);
    ct = cf2x_consts<Real>(c.physics);
    return memcmp(&rt, &ct, sizeof rt) == 0;
}

static bool config_is_cf2x(const adrp_config& c) {
    return c.precision ? is_cf2x<double>(c) : is_cf2x<float>(c);
}

template <typename Real>
static int upload_const(adrp_t* h) {
    const HoverConst<Real> k = hover_const<Real>(h->cfg);
    const HoverReset<Real> r = hover_reset_dist<Real>(h->cfg);
    if (hipMalloc(&h->cblk, sizeof k + sizeof r) != hipSuccess) return ADRP_ERR_OOM;
    if (hipMemcpy(h->cblk, &k, sizeof k, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((char*)h->cblk + sizeof k, &r, sizeof r, hipMemcpyHostToDevice) != hipSuccess)
        return ADRP_ERR_DEVICE;
    h->cf2x = is_cf2x<Real>(h->cfg);
    if (const char* env = getenv("ADRP_HOVER_GENERIC")) h->cf2x = h->cf2x && atoi(env) == 0;   // A/B: runtime constants
    return ADRP_OK;
}

// MultiHoverAviary: [HoverConst | HoverReset | MultiConst] (multihover_const)
template <typename Real>
static MultiConst<Real> multi_const(const adrp_config& c) {
    MultiConst<Real> m;
    memset(&m, 0, sizeof m);
    m.N = c.num_drones;
    m.dw1 = Real(c.drone.dw_coeff[0]); m.dw2 = Real(c.drone.dw_coeff[1]); m.dw3 = Real(c.drone.dw_coeff[2]);
    m.prop_r = Real(c.drone.prop_radius);
    for (int n = 0; n < c.num_drones; ++n)
        for (int j = 0; j < 3; ++j) {
            m.init_xyz[n][j] = Real(c.init_xyz[n][j]);
            m.init_rpy[n][j] = Real(c.init_rpy[n][j]);
            // TARGET_POS = INIT_XYZS + [0, 0, 1/(i+1)] in float64 (MultiHoverAviary.py:71)
            m.target[n][j] = Real(c.init_xyz[n][j] + (j == 2 ? 1.0 / (n + 1) : 0.0));
        }
    return m;
}

// X: MultiConst (MultiHoverAviary) or CtrlConst (CtrlAviary / VelocityAviary)
template <typename Real, typename X>
static int upload_multi_block(adrp_t* h, const X& m) {
    const HoverConst<Real> k = hover_const<Real>(h->cfg);
    const HoverReset<Real> r = hover_reset_dist<Real>(h->cfg);
    const size_t off = multihover_const_offset<Real>();
    if (hipMalloc(&h->cblk, off + sizeof m) != hipSuccess) return ADRP_ERR_OOM;
    if (hipMemcpy(h->cblk, &k, sizeof k, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((char*)h->cblk + sizeof k, &r, sizeof r, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((char*)h->cblk + off, &m, sizeof m, hipMemcpyHostToDevice) != hipSuccess)
        return ADRP_ERR_DEVICE;
    return ADRP_OK;
}

template <typename Real>
static int upload_multihover_const(adrp_t* h) {
    return upload_multi_block<Real>(h, multi_const<Real>(h->cfg));
}

static double max_rpm(const adrp_config& c) {   // BaseAviary.py:120
    const double gravity = c.gravity * c.drone.m;   // GRAVITY = G M first, as the reference rounds it
    return sqrt((c.drone.thrust2weight * gravity) / (4 * c.drone.kf));
}

template <typename Real>
static int upload_ctrl_const(adrp_t* h) {
    CtrlConst<Real> k;
    memset(&k, 0, sizeof k);
    k.m = multi_const<Real>(h->cfg);
    k.max_rpm = Real(max_rpm(h->cfg));
    return upload_multi_block<Real>(h, k);
}

template <typename Real>
static RaceConst<Real> race_const(const adrp_config& c) {
    const adrp_drone_params& d = c.drone;
    const adrp_track& t = c.track;
    RaceConst<Real> k;
    memset(&k, 0, sizeof k);
    k.N = c.num_drones;
    k.S = c.pyb_freq / c.ctrl_freq;
    k.physics = c.physics;
    k.link_lag = c.link_frame_lag ? 1 : 0;
    k.compete = c.race_mode == ADRP_RACE_COMPETE;
    k.num_gates = t.num_gates;
    k.num_obstacles = t.num_obstacles;
    k.trunc_steps = trunc_steps(t.episode_len_sec, c.pyb_freq);
    k.disturbances = t.disturbances ? 1 : 0;
    k.reward_wrapper = t.reward_wrapper ? 1 : 0;
    k.obs_wrapper = t.obs_wrapper == 1 || t.obs_wrapper == 2 ? t.obs_wrapper : 0;
    race_gyro_lpf(k.lpf);   // lpf2pInit(gyrolpf, 500, 30), adrp_internal.h
    k.random_gates = t.random_gates_obstacles ? 1 : 0;
    k.random_state = t.random_drone_state ? 1 : 0;
    k.random_inertia = t.random_drone_inertia ? 1 : 0;
    k.D = 49 + (k.compete ? 6 * (c.num_drones - 1) : 0);
    k.autoreset = c.autoreset ? 1 : 0;
    k.dt = Real(1.0 / c.pyb_freq);
    k.gravity = Real(c.gravity);
    k.kf = Real(d.kf); k.km = Real(d.km);
    for (int i = 0; i < 4; ++i) {
        k.px[i] = Real(d.prop_pos[i][0]); k.py[i] = Real(d.prop_pos[i][1]); k.pz[i] = Real(d.prop_pos[i][2]);
    }
    double hover_rpm, gnd_clip;
    derived(c, &hover_rpm, &gnd_clip);
    k.gnd_kf = Real(d.kf * d.gnd_eff_coeff);
    k.prop_r4 = Real(d.prop_radius / 4);
    k.gnd_clip = Real(gnd_clip);
    for (int i = 0; i < 3; ++i) k.drag[i] = Real(d.drag_coeff[i]);
    k.dw1 = Real(d.dw_coeff[0]); k.dw2 = Real(d.dw_coeff[1]); k.dw3 = Real(d.dw_coeff[2]);
    k.prop_r = Real(d.prop_radius);
    k.dyn_mass = Real(d.m); k.dyn_inv_mass = Real(1.0 / d.m);
    k.dyn_i[0] = Real(d.ixx); k.dyn_i[1] = Real(d.iyy); k.dyn_i[2] = Real(d.izz);
    k.dyn_inv_i[0] = Real(1.0 / d.ixx); k.dyn_inv_i[1] = Real(1.0 / d.iyy); k.dyn_inv_i[2] = Real(1.0 / d.izz);
    k.dyn_arm = Real(d.l / sqrt(2.0));
    k.coll_hh = Real(0.5 * d.collision_h); k.coll_r = Real(d.collision_r); k.coll_zoff = Real(d.collision_z_offset);
    k.ang_max = Real(0.5 * (M_PI / 2) * c.pyb_freq);
    for (int g = 0; g < ADRP_MAX_GATES; ++g) {
        k.gate_nom[g][0] = Real(t.gates[g][0]); k.gate_nom[g][1] = Real(t.gates[g][1]);
        k.gate_nom[g][2] = Real(t.gates[g][2]); k.gate_nom[g][3] = Real(t.gates[g][5]);
        k.gate_type[g] = t.gates[g][6] > 0 ? 1 : 0;
    }
    for (int o = 0; o < ADRP_MAX_OBSTACLES; ++o)
        for (int j = 0; j < 3; ++j) k.obst_nom[o][j] = Real(t.obstacles[o][j]);
    for (int j = 0; j < 3; ++j) {
        k.bounds[j] = Real(t.bounds_hi[j]);
        k.dist_lo[j] = Real(t.dyn_dist_low[j]); k.dist_hi[j] = Real(t.dyn_dist_high[j]);
        for (int m = 0; m < 2; ++m) { k.pos_off[j][m] = Real(t.pos_offset_range[j][m]); k.rot_off[j][m] = Real(t.rot_offset_range[j][m]); }
    }
    k.noise_std = Real(t.action_noise_std);
    for (int m = 0; m < 2; ++m) { k.gate_off[m] = Real(t.gate_offset_range[m]); k.obst_off[m] = Real(t.obstacle_offset_range[m]); }
    for (int j = 0; j < 4; ++j)
        for (int m = 0; m < 2; ++m) k.inertia_off[j][m] = Real(t.inertia_offset_range[j][m]);
    for (int i = 0; i < ADRP_MAX_DRONES; ++i)
        for (int j = 0; j < 3; ++j) {
            k.init_pos[i][j] = Real(t.init_pos[i][j]); k.init_rpy[i][j] = Real(t.init_rpy[i][j]);
            k.init_vel[i][j] = Real(t.init_vel[i][j]); k.init_pqr[i][j] = Real(t.init_pqr[i][j]);
        }
    k.race_mass = Real(t.race_mass);
    for (int j = 0; j < 3; ++j) k.race_inertia[j] = Real(t.race_inertia[j]);
    return k;
}

// the race drone's physical constants are race_cf2x_phys' bit for bit (the four-lane kernel's literals)
// (field by field, bitwise: a whole-struct memcmp would also compare padding bytes, which a struct
// copy need not preserve)
template <typename Real>
static bool race_is_cf2x(const RaceConst<Real>& rt) {
    RaceConst<Real> ct;
    memset(&ct, 0, sizeof ct);
    race_cf2x_phys(ct);
    bool same = true;
#define ADRP_SAME(f) same = same && memcmp(&rt.f, &ct.f, sizeof rt.f) == 0
    ADRP_SAME(dt); ADRP_SAME(gravity); ADRP_SAME(kf); ADRP_SAME(km);
    ADRP_SAME(px); ADRP_SAME(py); ADRP_SAME(pz);
    ADRP_SAME(gnd_kf); ADRP_SAME(prop_r4); ADRP_SAME(gnd_clip); ADRP_SAME(drag);
    ADRP_SAME(dw1); ADRP_SAME(dw2); ADRP_SAME(dw3); ADRP_SAME(prop_r);
    ADRP_SAME(dyn_mass); ADRP_SAME(dyn_inv_mass); ADRP_SAME(dyn_i); ADRP_SAME(dyn_inv_i); ADRP_SAME(dyn_arm);
    ADRP_SAME(coll_hh); ADRP_SAME(coll_r); ADRP_SAME(coll_zoff); ADRP_SAME(ang_max); ADRP_SAME(link_lag);
#undef ADRP_SAME
    return same;
}

template <typename Real>
static int upload_race_const(adrp_t* h) {
    RaceConst<Real> k = race_const<Real>(h->cfg);
    k.refine = h->race_refine ? 1 : 0;
    h->race_cf2x = race_is_cf2x(k);
    // [RaceConst | tick-schedule tables (att, pos)] (race_args)
    std::vector<uint32_t> ticks(2 * kTickWords);
    race_tick_tables(ticks.data(), ticks.data() + kTickWords);
    const size_t off = race_ticks_offset<Real>();
    if (!h->cblk && hipMalloc(&h->cblk, off + ticks.size() * 4) != hipSuccess) return ADRP_ERR_OOM;
    if (hipMemcpy(h->cblk, &k, sizeof k, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((char*)h->cblk + off, ticks.data(), ticks.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return ADRP_ERR_DEVICE;
    // the nominal attitudes, with the kernels' own transcendentals (RaceConst::nom_q / nom_rpy)
    hipLaunchKernelGGL(race_const_init_kernel<Real>, dim3(1), dim3(64), 0, 0, (RaceConst<Real>*)h->cblk);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ADRP_ERR_DEVICE;
    return ADRP_OK;
}


extern "C" const char* adrp_kernel_name(const adrp_config* cfg) {
    static thread_local char buf[96];
    if (!cfg || cfg->struct_size != sizeof(adrp_config)) return nullptr;
    static const char* ph[] = {"PYB", "DYN", "PYB_GND", "PYB_DRAG", "PYB_DW", "PYB_GND_DRAG_DW"};
    const int p = cfg->physics >= 0 && cfg->physics <= 5 ? cfg->physics : 0;
    if (cfg->task == ADRP_TASK_RACE) {
        const char* q = getenv("ADRP_RACE_QUAD");
        const bool cf2x = cfg->precision ? race_is_cf2x(race_const<double>(*cfg)) : race_is_cf2x(race_const<float>(*cfg));
        const char* pd = getenv("ADRP_RACE_PREDRAW");
        const int S = cfg->ctrl_freq > 0 ? cfg->pyb_freq / cfg->ctrl_freq : 0;
        const bool quad = !(q && atoi(q) == 0) && (cf2x || !cfg->precision) &&
                          !(cfg->track.disturbances && (S > kRacePreS || (pd && atoi(pd) == 0)));
        snprintf(buf, sizeof buf, "race_step<%s,%s,G%d%s>", cfg->precision ? "f64" : "f32", ph[p],
                 race_group(cfg->num_drones), quad ? ",Q4" : "");
        return buf;
    }
    if (is_ctrl_task(cfg->task)) {
        snprintf(buf, sizeof buf, "%s_step<%s,%s,G%d>", cfg->task == ADRP_TASK_CTRL ? "ctrl" : "velocity",
                 cfg->precision ? "f64" : "f32", ph[p], mh_group(cfg->num_drones));
        return buf;
    }
    const int A = hover_act_dim(cfg->act_type);
    if (cfg->task == ADRP_TASK_MULTIHOVER) {
        snprintf(buf, sizeof buf, "multihover_step<%s,%s,A%d,G%d>", cfg->precision ? "f64" : "f32", ph[p], A,
                 mh_group(cfg->num_drones));
        return buf;
    }
    if (hover_has_pid(cfg->act_type)) {
        static const char* ctl[] = {"", "", "", "PID", "VEL", "ONE_D_PID"};
        snprintf(buf, sizeof buf, "hover_step<%s,%s,A%d,Bn,generic,%s>", cfg->precision ? "f64" : "f32", ph[p], A,
                 ctl[cfg->act_type]);
        return buf;
    }
    snprintf(buf, sizeof buf, "hover_step<%s,%s,A%d,B%s,%s>", cfg->precision ? "f64" : "f32", ph[p], A,
             cfg->action_buffer_size == 15 ? "15" : "n", config_is_cf2x(*cfg) ? "cf2x" : "generic");
    return buf;
}

// the instantiation a live handle launches: command mode (adrp_enable_commands) switches a race
// handle to the one-lane G = 8 command kernel, ADRP_RACE_QUAD is read at create
extern "C" const char* adrp_handle_kernel_name(const adrp_t* h) {
    static thread_local char buf[96];
    if (!h) return nullptr;
    if (h->cfg.task != ADRP_TASK_RACE) {
        const char* n = adrp_kernel_name(&h->cfg);
        const char* c = strstr(n, ",cf2x>");
        if (!c || h->cf2x) return n;
        snprintf(buf, sizeof buf, "%.*s,generic>", int(c - n), n);   // ADRP_HOVER_GENERIC
        return buf;
    }
    static const char* ph[] = {"PYB", "DYN", "PYB_GND", "PYB_DRAG", "PYB_DW", "PYB_GND_DRAG_DW"};
    const int p = h->cfg.physics >= 0 && h->cfg.physics <= 5 ? h->cfg.physics : 0;
    const char* prec = h->real_size == 8 ? "f64" : "f32";
    if (h->cmdf) snprintf(buf, sizeof buf, "race_step<%s,%s,G8,CMD>", prec, ph[p]);
    else snprintf(buf, sizeof buf, "race_step<%s,%s,G%d%s>", prec, ph[p], race_group(h->N),
                  race_quad_ok(h) ? ",Q4" : "");
    return buf;
}

// ---------------------------------------------------------------------------------------------
extern "C" int adrp_create(const adrp_config* cfg, int device, adrp_t** out) {
    if (!out) return seterr(nullptr, ADRP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adrp_config))
        return seterr(nullptr, ADRP_ERR_INVALID, "adrp_config.struct_size mismatch (ABI)");
    const adrp_config& c = *cfg;
    if (c.num_envs <= 0) return seterr(nullptr, ADRP_ERR_INVALID, "num_envs must be > 0");
    if (c.ctrl_freq <= 0 || c.pyb_freq <= 0 || c.pyb_freq % c.ctrl_freq != 0)
        return seterr(nullptr, ADRP_ERR_INVALID, "pyb_freq is not divisible by env_freq");  // BaseAviary.py:79-80
    if (c.physics < ADRP_PHYS_PYB || c.physics > ADRP_PHYS_PYB_GND_DRAG_DW)
        return seterr(nullptr, ADRP_ERR_INVALID, "unknown physics");
    if (c.precision != 0 && c.precision != 1) return seterr(nullptr, ADRP_ERR_INVALID, "precision must be 0 or 1");
    if (c.task == ADRP_TASK_HOVER) {
        if (c.num_drones != 1) return seterr(nullptr, ADRP_ERR_INVALID, "HoverAviary has exactly one drone");
        if (c.act_type != ADRP_ACT_RPM && c.act_type != ADRP_ACT_ONE_D_RPM && !hover_has_pid(c.act_type))
            return seterr(nullptr, ADRP_ERR_INVALID, "HoverAviary act_type must be RPM, ONE_D_RPM, PID, VEL or ONE_D_PID");
        if (c.action_buffer_size <= 0 || c.action_buffer_size > 4096)
            return seterr(nullptr, ADRP_ERR_INVALID, "action_buffer_size");
    } else if (c.task == ADRP_TASK_MULTIHOVER) {
        if (c.num_drones < 1 || c.num_drones > ADRP_MAX_DRONES)
            return seterr(nullptr, ADRP_ERR_INVALID, "MultiHoverAviary num_drones must be 1..8");
        if (hover_has_pid(c.act_type))
            return seterr(nullptr, ADRP_ERR_INVALID, "MultiHoverAviary act_type PID, VEL and ONE_D_PID are not supported "
                                                     "(RPM or ONE_D_RPM)");
        if (c.act_type != ADRP_ACT_RPM && c.act_type != ADRP_ACT_ONE_D_RPM)
            return seterr(nullptr, ADRP_ERR_INVALID, "MultiHoverAviary act_type must be RPM or ONE_D_RPM");
        if (c.action_buffer_size <= 0 || c.action_buffer_size > 4096)
            return seterr(nullptr, ADRP_ERR_INVALID, "action_buffer_size");
    } else if (c.task == ADRP_TASK_CTRL) {
        if (c.num_drones < 1 || c.num_drones > ADRP_MAX_DRONES)
            return seterr(nullptr, ADRP_ERR_INVALID, "CtrlAviary num_drones must be 1..8");
        if (c.act_type != ADRP_ACT_RAW_RPM) return seterr(nullptr, ADRP_ERR_INVALID, "CtrlAviary act_type must be RAW_RPM");
    } else if (c.task == ADRP_TASK_VELOCITY) {
        if (c.num_drones < 1 || c.num_drones > ADRP_MAX_DRONES)
            return seterr(nullptr, ADRP_ERR_INVALID, "VelocityAviary num_drones must be 1..8");
        if (c.act_type != ADRP_ACT_VEL) return seterr(nullptr, ADRP_ERR_INVALID, "VelocityAviary act_type must be VEL");
    } else if (c.task == ADRP_TASK_RACE) {
        if (c.num_drones < 1 || c.num_drones > ADRP_MAX_DRONES)
            return seterr(nullptr, ADRP_ERR_INVALID, "MultiRaceAviary num_drones must be 1..8");
        if (c.act_type != ADRP_ACT_FULLSTATE)
            return seterr(nullptr, ADRP_ERR_INVALID, "MultiRaceAviary act_type must be FULLSTATE");
        if (c.race_mode != ADRP_RACE_COMPARE && c.race_mode != ADRP_RACE_COMPETE)
            return seterr(nullptr, ADRP_ERR_INVALID, "race_mode");
        if (c.track.num_gates < 0 || c.track.num_gates > ADRP_MAX_GATES || c.track.num_obstacles < 0 ||
            c.track.num_obstacles > ADRP_MAX_OBSTACLES)
            return seterr(nullptr, ADRP_ERR_INVALID, "track: at most 4 gates and 4 obstacles (MultiRaceAviary.py:591-651)");
    } else {
        return seterr(nullptr, ADRP_ERR_INVALID, "unknown task");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return seterr(nullptr, ADRP_ERR_DEVICE, "no HIP device visible (libadrp has no CPU fallback)");
    if (device < 0 || device >= ndev) return seterr(nullptr, ADRP_ERR_INVALID, "device index out of range");
    adrp_t* h = new adrp_t();
    h->cfg = c;
    h->device = device;
    h->E = c.num_envs; h->N = c.num_drones;
    const bool race = c.task == ADRP_TASK_RACE;
    const bool ctrl = is_ctrl_task(c.task);   // no action history: no ring, action_buffer_size is not read
    h->A = race || ctrl ? 4 : hover_act_dim(c.act_type);
    h->B = race || ctrl ? 0 : c.action_buffer_size;
    h->D = race ? 49 + (c.race_mode == ADRP_RACE_COMPETE ? 6 * (c.num_drones - 1) : 0)
                : ctrl ? kCtrlObs : 12 + h->B * h->A;
    h->S = c.pyb_freq / c.ctrl_freq;
    h->nf_base = race ? RF_N : HF_NBASE + (hover_has_pid(c.act_type) ? HF_NPID : 0);
    h->ni = race ? RI_N : HI_N;
    h->real_size = c.precision ? 8 : 4;
    const size_t EN = size_t(h->E) * h->N;
    auto cleanup = [&](int rc) {
        hipFree(h->f); hipFree(h->ring); hipFree(h->ist); hipFree(h->counters); hipFree(h->cblk);
        hipFree(h->img_f); hipFree(h->img_i); hipFree(h->img_row); hipFree(h->img_ep);
        g_err = h->err;
        delete h;
        return rc;
    };
    DeviceGuard g(device);
    const size_t ring_bytes = size_t(h->B) * h->A * EN * sizeof(float);   // [B][E*N][A] (race: none)
    if (hipMalloc(&h->f, h->nf_base * EN * h->real_size) != hipSuccess ||
        (ring_bytes && hipMalloc((void**)&h->ring, ring_bytes) != hipSuccess) ||
        hipMalloc((void**)&h->ist, h->ni * EN * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&h->counters, 64 * sizeof(int32_t)) != hipSuccess)
        return cleanup(seterr(h, ADRP_ERR_OOM, "hipMalloc failed"));
    if (hipMemset(h->f, 0, h->nf_base * EN * h->real_size) != hipSuccess ||
        (ring_bytes && hipMemset(h->ring, 0, ring_bytes) != hipSuccess) ||
        hipMemset(h->ist, 0, h->ni * EN * sizeof(int32_t)) != hipSuccess ||
        hipMemset(h->counters, 0, 64 * sizeof(int32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return cleanup(seterr(h, ADRP_ERR_DEVICE, "initialisation failed"));
    if (const char* env = getenv("ADRP_STAGE_ROWS")) h->stage_rows = atoi(env) != 0;
    if (const char* env = getenv("ADRP_RESET_HELPER")) h->reset_helper = atoi(env) != 0;
    if (const char* env = getenv("ADRP_RACE_HELPERS")) h->race_helpers = atoi(env) != 0;
    if (const char* env = getenv("ADRP_RACE_QUAD")) h->race_quad = atoi(env) != 0;
    if (const char* env = getenv("ADRP_RACE_REFINE")) h->race_refine = atoi(env) != 0;
    if (const char* env = getenv("ADRP_RACE_PREDRAW")) h->race_predraw = atoi(env) != 0;
    const int rc = race ? (h->real_size == 8 ? upload_race_const<double>(h) : upload_race_const<float>(h))
                   : c.task == ADRP_TASK_MULTIHOVER
                        ? (h->real_size == 8 ? upload_multihover_const<double>(h) : upload_multihover_const<float>(h))
                   : ctrl ? (h->real_size == 8 ? upload_ctrl_const<double>(h) : upload_ctrl_const<float>(h))
                        : (h->real_size == 8 ? upload_const<double>(h) : upload_const<float>(h));
    if (rc != ADRP_OK) return cleanup(seterr(h, rc, "constant block upload failed"));
    if (const char* env = getenv("ADRP_RESET_IMAGES")) h->img_period = atoi(env);
    if (race && c.autoreset && h->img_period > 0) {   // next-reset images (race_quad.h)
        if (hipMalloc(&h->img_f, size_t(RF_N) * EN * h->real_size) != hipSuccess ||
            hipMalloc((void**)&h->img_i, size_t(RI_N) * EN * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void**)&h->img_row, EN * size_t(h->D) * sizeof(float)) != hipSuccess ||
            hipMalloc((void**)&h->img_ep, size_t(h->E) * sizeof(int32_t)) != hipSuccess)
            return cleanup(seterr(h, ADRP_ERR_OOM, "hipMalloc failed (reset images)"));
        if (hipMemset(h->img_ep, 0xff, size_t(h->E) * sizeof(int32_t)) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess)
            return cleanup(seterr(h, ADRP_ERR_DEVICE, "initialisation failed (reset images)"));
    }
    *out = h;
    return ADRP_OK;
}

extern "C" void adrp_destroy(adrp_t* h) {
    if (!h) return;
    if (h->pbox) adrp_persistent_end(h);
    DeviceGuard g(h->device);
    hipDeviceSynchronize();
    for (auto e : h->ev_start) hipEventDestroy(e);
    for (auto e : h->ev_stop) hipEventDestroy(e);
    hipFree(h->f); hipFree(h->ring); hipFree(h->ist); hipFree(h->counters); hipFree(h->cblk);
    hipFree(h->cmdf); hipFree(h->cmdi); hipFree(h->mom_hash); hipFree(h->mom_log); hipFree(h->mom_log_n);
    hipFree(h->img_f); hipFree(h->img_i); hipFree(h->img_row); hipFree(h->img_ep);
    delete h;
}

// next-reset images are keyed by the episode; a new seed or constant block makes them all stale
static int images_invalidate(adrp_t* h, hipStream_t s) {
    if (!h->img_ep) return ADRP_OK;
    HIPCHK(h, hipMemsetAsync(h->img_ep, 0xff, size_t(h->E) * sizeof(int32_t), s));
    h->img_ctr = 0;   // the next step refills
    return ADRP_OK;
}

extern "C" int adrp_reseed(adrp_t* h, uint64_t seed, void* stream) {
    if (!h) return seterr(h, ADRP_ERR_INVALID, "adrp_reseed: NULL handle");
    // the resident kernel owns the episode counters and fixed its seed at launch: refuse
    // before any change (a half-applied reseed would race with it)
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_reseed: persistent mode is active (adrp_persistent_end first)");
    DeviceGuard g(h->device);
    h->cfg.seed = seed;   // read into the kernel arguments at every launch
    const size_t EN = size_t(h->E) * h->N;
    static_assert(RI_EPISODE == 1 && HI_EPISODE == 1, "episode counters are int row 1 in both tasks");
    HIPCHK(h, hipMemsetAsync(h->ist + EN, 0, EN * sizeof(int32_t), (hipStream_t)stream));
    return images_invalidate(h, (hipStream_t)stream);
}

extern "C" int adrp_set_wrappers(adrp_t* h, int reward_wrapper, int obs_wrapper) {
    if (!h) return seterr(h, ADRP_ERR_INVALID, "adrp_set_wrappers: NULL handle");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_set_wrappers: persistent mode is active (adrp_persistent_end first)");
    if (h->cfg.task != ADRP_TASK_RACE) return seterr(h, ADRP_ERR_INVALID, "wrappers are MultiRaceAviary's");
    if (obs_wrapper < 0 || obs_wrapper > 2) return seterr(h, ADRP_ERR_INVALID, "obs_wrapper must be 0, 1 or 2");
    DeviceGuard g(h->device);
    HIPCHK(h, hipDeviceSynchronize());   // no step in flight reads the old block
    h->cfg.track.reward_wrapper = reward_wrapper ? 1 : 0;
    h->cfg.track.obs_wrapper = obs_wrapper;
    const int rc = h->real_size == 8 ? upload_race_const<double>(h) : upload_race_const<float>(h);
    if (rc != ADRP_OK) return seterr(h, rc, "constant block upload failed");
    return images_invalidate(h, nullptr);
}

extern "C" int adrp_set_noise(adrp_t* h, const double* act_noise_dev, const double* force_dev) {
    if (!h) return seterr(h, ADRP_ERR_INVALID, "adrp_set_noise: NULL handle");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_set_noise: persistent mode is active (adrp_persistent_end first)");
    if (h->cfg.task != ADRP_TASK_RACE) return seterr(h, ADRP_ERR_INVALID, "noise injection is MultiRaceAviary's");
    if ((act_noise_dev == nullptr) != (force_dev == nullptr))
        return seterr(h, ADRP_ERR_INVALID, "adrp_set_noise: both arrays or neither");
    h->inj_act = act_noise_dev;
    h->inj_force = force_dev;
    return ADRP_OK;
}

extern "C" int adrp_obs_dim(const adrp_t* h) { return h ? h->D : ADRP_ERR_INVALID; }
extern "C" int adrp_act_dim(const adrp_t* h) { return h ? h->A : ADRP_ERR_INVALID; }

extern "C" int adrp_reset(adrp_t* h, const uint8_t* env_mask_dev, float* obs_dev, void* stream) {
    if (!h || !obs_dev) return seterr(h, ADRP_ERR_INVALID, "adrp_reset: NULL argument");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_reset: persistent mode is active (adrp_persistent_end first)");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->cfg.task == ADRP_TASK_RACE) {
        h->img_ctr = 0;   // the next step refills the next-reset images of the new episodes
        return h->real_size == 8 ? race_reset<double>(h, env_mask_dev, obs_dev, s)
                                 : race_reset<float>(h, env_mask_dev, obs_dev, s);
    }
    if (h->cfg.task == ADRP_TASK_MULTIHOVER)
        return h->real_size == 8 ? multihover_reset<double>(h, env_mask_dev, obs_dev, s)
                                 : multihover_reset<float>(h, env_mask_dev, obs_dev, s);
    if (is_ctrl_task(h->cfg.task))
        return h->real_size == 8 ? ctrl_reset<double>(h, env_mask_dev, obs_dev, s)
                                 : ctrl_reset<float>(h, env_mask_dev, obs_dev, s);
    return h->real_size == 8 ? hover_reset<double>(h, env_mask_dev, obs_dev, s)
                             : hover_reset<float>(h, env_mask_dev, obs_dev, s);
}

extern "C" int adrp_step(adrp_t* h, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* term_dev,
                         uint8_t* trunc_dev, float* terminal_obs_dev, void* stream) {
    if (!h || (!act_dev && !h->cmdf) || !obs_dev || !rew_dev || !term_dev || !trunc_dev)
        return seterr(h, ADRP_ERR_INVALID, "adrp_step: NULL argument");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_step: persistent mode is active (adrp_persistent_step)");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    if (h->cfg.task == ADRP_TASK_RACE)
        return h->real_size == 8 ? race_step<double>(h, act_dev, obs_dev, rew_dev, term_dev, trunc_dev, terminal_obs_dev, s)
                                 : race_step<float>(h, act_dev, obs_dev, rew_dev, term_dev, trunc_dev, terminal_obs_dev, s);
    if (h->cfg.task == ADRP_TASK_MULTIHOVER)
        return h->real_size == 8 ? multihover_step<double>(h, act_dev, obs_dev, rew_dev, term_dev, trunc_dev, terminal_obs_dev, s)
                                 : multihover_step<float>(h, act_dev, obs_dev, rew_dev, term_dev, trunc_dev, terminal_obs_dev, s);
    if (is_ctrl_task(h->cfg.task))   // (no episode ends: terminal_obs_dev is never written)
        return h->real_size == 8 ? ctrl_step<double>(h, act_dev, nullptr, obs_dev, rew_dev, term_dev, trunc_dev, s)
                                 : ctrl_step<float>(h, act_dev, nullptr, obs_dev, rew_dev, term_dev, trunc_dev, s);
    return h->real_size == 8 ? hover_step<double>(h, act_dev, obs_dev, rew_dev, term_dev, trunc_dev, terminal_obs_dev, s)
                             : hover_step<float>(h, act_dev, obs_dev, rew_dev, term_dev, trunc_dev, terminal_obs_dev, s);
}

extern "C" int adrp_step_rpm(adrp_t* h, const void* rpm_dev, float* obs_dev, float* rew_dev, uint8_t* term_dev,
                             uint8_t* trunc_dev, void* stream) {
    if (!h || !rpm_dev || !obs_dev || !rew_dev || !term_dev || !trunc_dev)
        return seterr(h, ADRP_ERR_INVALID, "adrp_step_rpm: NULL argument");
    if (h->cfg.task != ADRP_TASK_CTRL) return seterr(h, ADRP_ERR_INVALID, "adrp_step_rpm: CtrlAviary handles only");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    return h->real_size == 8 ? ctrl_step<double>(h, nullptr, rpm_dev, obs_dev, rew_dev, term_dev, trunc_dev, s)
                             : ctrl_step<float>(h, nullptr, rpm_dev, obs_dev, rew_dev, term_dev, trunc_dev, s);
}

// ---------------------------------------------------------------------------------------------
// SB3 host path in one call per step (vec_env.py): pinned host blocks mapped into the device
// ---------------------------------------------------------------------------------------------
int vec_compact_launch(const adrp_vec_io& d, int n, int rf, hipStream_t s);

extern "C" int adrp_vec_bind(adrp_t* h, int slot, const adrp_vec_io* io) {
    if (!h || !io || slot < 0 || slot >= ADRP_VEC_SLOTS) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: arguments");
    if (!io->act || !io->obs || !io->rew || !io->term || !io->trunc || !io->done || !io->count || !io->idx ||
        (io->cap > 0 && !io->rows) || io->cap < 0 || !io->term_dev || !io->trunc_dev || !io->tobs_dev || !io->idx_dev)
        return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: NULL pointer");
    DeviceGuard g(h->device);
    adrp_vec_io d = *io;
    // host addresses -> the device's view of the same pinned pages
    auto map = [&](const void* p, void** out) { return hipHostGetDevicePointer(out, const_cast<void*>(p), 0); };
    void* t = nullptr;
    if (map(io->act, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: act is not pinned host memory");
    d.act = (const float*)t;
    if (map(io->obs, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: obs is not pinned host memory");
    d.obs = (float*)t;
    if (map(io->rew, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: rew is not pinned host memory");
    d.rew = (float*)t;
    if (map(io->term, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: term is not pinned host memory");
    d.term = (uint8_t*)t;
    if (map(io->trunc, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: trunc is not pinned host memory");
    d.trunc = (uint8_t*)t;
    if (map(io->done, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: done is not pinned host memory");
    d.done = (uint8_t*)t;
    if (map(io->count, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: count is not pinned host memory");
    d.count = (int32_t*)t;
    if (map(io->idx, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: idx is not pinned host memory");
    d.idx = (int32_t*)t;
    if (io->cap > 0) {
        if (map(io->rows, &t) != hipSuccess) return seterr(h, ADRP_ERR_INVALID, "adrp_vec_bind: rows is not pinned host memory");
        d.rows = (float*)t;
    }
    h->vio[slot] = d;
    h->vbound[slot] = true;
    return ADRP_OK;
}

extern "C" int adrp_vec_step(adrp_t* h, int slot, void* stream) {
    if (!h || slot < 0 || slot >= ADRP_VEC_SLOTS || !h->vbound[slot])
        return seterr(h, ADRP_ERR_INVALID, "adrp_vec_step: slot not bound (adrp_vec_bind)");
    const adrp_vec_io& d = h->vio[slot];
    int rc = adrp_step(h, d.act, d.obs, d.rew, d.term_dev, d.trunc_dev, d.tobs_dev, stream);
    if (rc != ADRP_OK) return rc;
    DeviceGuard g(h->device);
    if (vec_compact_launch(d, h->E, h->N * h->D, (hipStream_t)stream) != ADRP_OK)
        return seterr(h, ADRP_ERR_DEVICE, "adrp_vec_step: compaction launch");
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    return ADRP_OK;
}

// ---------------------------------------------------------------------------------------------
// high-level command mode (commander.h)
// ---------------------------------------------------------------------------------------------
extern "C" int adrp_enable_commands(adrp_t* h) {
    if (!h) return seterr(h, ADRP_ERR_INVALID, "adrp_enable_commands: NULL handle");
    if (h->cfg.task != ADRP_TASK_RACE) return seterr(h, ADRP_ERR_INVALID, "commands are MultiRaceAviary's");
    if (h->cmdf) return ADRP_OK;
    DeviceGuard g(h->device);
    const size_t EN = size_t(h->E) * h->N;
    HIPCHK(h, hipDeviceSynchronize());   // no step in flight
    if (hipMalloc((void**)&h->cmdf, ADRP_CMD_NF * EN * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&h->cmdi, ADRP_CMD_NI * EN * sizeof(int32_t)) != hipSuccess) {
        hipFree(h->cmdf); hipFree(h->cmdi);
        h->cmdf = nullptr; h->cmdi = nullptr;
        return seterr(h, ADRP_ERR_OOM, "hipMalloc failed (command state)");
    }
    // what reset() leaves (MellingerControl.py:119-150): an idle planner, override on, an unset
    // setpoint, the commander at the nominal initial pose
    const int rc = h->real_size == 8 ? race_cmd_init<double>(h, nullptr) : race_cmd_init<float>(h, nullptr);
    if (rc != ADRP_OK) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    return ADRP_OK;
}

extern "C" int adrp_race_command(adrp_t* h, const int32_t* cmd_dev, const double* args_dev, void* stream) {
    if (!h || !cmd_dev || !args_dev) return seterr(h, ADRP_ERR_INVALID, "adrp_race_command: NULL argument");
    if (!h->cmdf) return seterr(h, ADRP_ERR_INVALID, "adrp_race_command: call adrp_enable_commands first");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    return h->real_size == 8 ? race_command<double>(h, cmd_dev, args_dev, s) : race_command<float>(h, cmd_dev, args_dev, s);
}

extern "C" int adrp_get_command_state(adrp_t* h, float* f_dev, int32_t* i_dev, void* stream) {
    if (!h || !f_dev || !i_dev) return seterr(h, ADRP_ERR_INVALID, "adrp_get_command_state: NULL argument");
    if (!h->cmdf) return seterr(h, ADRP_ERR_INVALID, "command mode is off (adrp_enable_commands)");
    DeviceGuard g(h->device);
    const size_t EN = size_t(h->E) * h->N;
    HIPCHK(h, hipMemcpyAsync(f_dev, h->cmdf, ADRP_CMD_NF * EN * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(h, hipMemcpyAsync(i_dev, h->cmdi, ADRP_CMD_NI * EN * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADRP_OK;
}

extern "C" int adrp_set_command_state(adrp_t* h, const float* f_dev, const int32_t* i_dev, void* stream) {
    if (!h || !f_dev || !i_dev) return seterr(h, ADRP_ERR_INVALID, "adrp_set_command_state: NULL argument");
    if (!h->cmdf) return seterr(h, ADRP_ERR_INVALID, "command mode is off (adrp_enable_commands)");
    DeviceGuard g(h->device);
    const size_t EN = size_t(h->E) * h->N;
    HIPCHK(h, hipMemcpyAsync(h->cmdf, f_dev, ADRP_CMD_NF * EN * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(h, hipMemcpyAsync(h->cmdi, i_dev, ADRP_CMD_NI * EN * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADRP_OK;
}

namespace adrp {
// snapshot <-> internal ring: user fields ring_{s}_{j} = [B*A][E] (physical slot s, per-env
// ring_head); internal [B][E][A].  Both keep the same physical slots and heads.
__global__ void ring_get_kernel(const float* __restrict__ ring, void* dst, int is_double, int B, int A, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    for (int s = 0; s < B; ++s)
        for (int j = 0; j < A; ++j) {
            const float v = ring[(size_t(s) * E + e) * A + j];
            const size_t o = size_t(s * A + j) * E + e;
            if (is_double) static_cast<double*>(dst)[o] = v;
            else static_cast<float*>(dst)[o] = v;
        }
}
__global__ void ring_set_kernel(float* __restrict__ ring, const void* src, int is_double, int B, int A, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    for (int s = 0; s < B; ++s)
        for (int j = 0; j < A; ++j) {
            const size_t o = size_t(s * A + j) * E + e;
            ring[(size_t(s) * E + e) * A + j] =
                is_double ? float(static_cast<const double*>(src)[o]) : static_cast<const float*>(src)[o];
        }
}

// MultiHoverAviary: the per-env ints are replicated on the env's N columns from drone 0's
__global__ void spread_ints_kernel(int32_t* __restrict__ ist, int ni, int E, int N) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const size_t EN = size_t(E) * N, c0 = size_t(e) * N;
    for (int k = 0; k < ni; ++k)
        for (int n = 1; n < N; ++n) ist[k * EN + c0 + n] = ist[k * EN + c0];
}

}  // namespace adrp

// ---------------------------------------------------------------------------------------------
// state snapshot
// ---------------------------------------------------------------------------------------------
static const char* k_hover_f[HF_NBASE] = {
    "pos_x", "pos_y", "pos_z", "quat_x", "quat_y", "quat_z", "quat_w", "vel_x", "vel_y", "vel_z",
    "omega_x", "omega_y", "omega_z", "last_rpm_0", "last_rpm_1", "last_rpm_2", "last_rpm_3",
    "angv_x", "angv_y", "angv_z", "link_quat_x", "link_quat_y", "link_quat_z", "link_quat_w"};
static const char* k_hover_i[HI_N] = {"step_counter", "episode", "ring_head"};
static const char* k_hover_pid[HF_NPID] = {"pid_last_rpy_x", "pid_last_rpy_y", "pid_last_rpy_z",
                                           "pid_int_pos_x", "pid_int_pos_y", "pid_int_pos_z",
                                           "pid_int_rpy_x", "pid_int_rpy_y", "pid_int_rpy_z"};

extern "C" int adrp_state_layout(const adrp_t* h, int* nf, int* ni) {
    if (!h || !nf || !ni) return ADRP_ERR_INVALID;
    *nf = h->nf_base + h->B * h->A;
    *ni = h->ni;
    return ADRP_OK;
}

static const char* k_race_f[64] = {
    "pos_x", "pos_y", "pos_z", "quat_x", "quat_y", "quat_z", "quat_w", "vel_x", "vel_y", "vel_z",
    "omega_x", "omega_y", "omega_z", "rpm_0", "rpm_1", "rpm_2", "rpm_3", "prev_rpm_0", "prev_rpm_1",
    "prev_rpm_2", "prev_rpm_3", "angv_x", "angv_y", "angv_z", "link_quat_x", "link_quat_y", "link_quat_z",
    "link_quat_w", "link_pos_x", "link_pos_y", "link_pos_z", "kin_pos_x", "kin_pos_y", "kin_pos_z",
    "prev_rpy_0", "prev_rpy_1", "prev_rpy_2", "prev_vel_0", "prev_vel_1", "prev_vel_2",
    "lpf_d1_0", "lpf_d1_1", "lpf_d1_2", "lpf_d2_0", "lpf_d2_1", "lpf_d2_2",
    "i_err_0", "i_err_1", "i_err_2", "i_err_m_0", "i_err_m_1", "i_err_m_2",
    "prev_omega_roll", "prev_omega_pitch", "prev_sp_roll", "prev_sp_pitch",
    "ctl_roll", "ctl_pitch", "ctl_yaw", "ctl_thrust", "mass", "ixx", "iyy", "izz"};
static const char* k_race_i[RI_N] = {"step_counter", "episode", "tick", "last_att_tick", "last_pos_tick",
                                     "tumble", "gate", "flags", "wr_gate"};

extern "C" const char* adrp_state_field(const adrp_t* h, int is_int, int index) {
    static thread_local char buf[32];
    if (!h || index < 0) return nullptr;
    if (h->cfg.task == ADRP_TASK_RACE) {
        if (is_int) return index < RI_N ? k_race_i[index] : nullptr;
        if (index < 64) return k_race_f[index];
        static const char* gc[4] = {"x", "y", "z", "yaw"};
        static const char* oc[3] = {"x", "y", "z"};
        if (index < 80) snprintf(buf, sizeof buf, "gate_%d_%s", (index - 64) / 4, gc[(index - 64) % 4]);
        else if (index < 92) snprintf(buf, sizeof buf, "obst_%d_%s", (index - 80) / 3, oc[(index - 80) % 3]);
        else if (index < 95) snprintf(buf, sizeof buf, "wr_target_%d", index - 92);
        else if (index < RF_N) snprintf(buf, sizeof buf, "wr_prev_%d", index - 95);
        else return nullptr;
        return buf;
    }
    if (is_int) return index < h->ni ? k_hover_i[index] : nullptr;
    if (index < HF_NBASE) return k_hover_f[index];
    if (index < h->nf_base) return k_hover_pid[index - HF_NBASE];
    const int k = index - h->nf_base;
    if (k >= h->B * h->A) return nullptr;
    snprintf(buf, sizeof buf, "ring_%d_%d", k / h->A, k % h->A);
    return buf;
}

extern "C" int adrp_get_state(adrp_t* h, void* f_dev, int32_t* i_dev, void* stream) {
    if (!h || !f_dev || !i_dev) return seterr(h, ADRP_ERR_INVALID, "adrp_get_state: NULL argument");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_get_state: persistent mode is active (adrp_persistent_end first)");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t EN = size_t(h->E) * h->N, nb = h->nf_base * EN, nr = size_t(h->B) * h->A * h->E;
    HIPCHK(h, hipMemcpyAsync(f_dev, h->f, nb * h->real_size, hipMemcpyDeviceToDevice, s));
    void* ring_dst = (char*)f_dev + nb * h->real_size;
    // (the ring has one column per drone: E*N of them for MultiHoverAviary, N = 1 for HoverAviary)
    if (h->B > 0) hipLaunchKernelGGL(ring_get_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, s, h->ring, ring_dst,
                       int(h->real_size == 8), h->B, h->A, int(EN));
    HIPCHK(h, hipGetLastError());
    (void)nr;
    HIPCHK(h, hipMemcpyAsync(i_dev, h->ist, h->ni * EN * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return ADRP_OK;
}

extern "C" int adrp_set_state(adrp_t* h, const void* f_dev, const int32_t* i_dev, void* stream) {
    if (!h || !f_dev || !i_dev) return seterr(h, ADRP_ERR_INVALID, "adrp_set_state: NULL argument");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_set_state: persistent mode is active (adrp_persistent_end first)");
    DeviceGuard g(h->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t EN = size_t(h->E) * h->N, nb = h->nf_base * EN, nr = size_t(h->B) * h->A * h->E;
    HIPCHK(h, hipMemcpyAsync(h->f, f_dev, nb * h->real_size, hipMemcpyDeviceToDevice, s));
    const void* ring_src = (const char*)f_dev + nb * h->real_size;
    if (h->B > 0) hipLaunchKernelGGL(ring_set_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, s, h->ring, ring_src,
                       int(h->real_size == 8), h->B, h->A, int(EN));
    HIPCHK(h, hipGetLastError());
    (void)nr;
    HIPCHK(h, hipMemcpyAsync(h->ist, i_dev, h->ni * EN * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if ((h->cfg.task == ADRP_TASK_MULTIHOVER || is_ctrl_task(h->cfg.task)) && h->N > 1) {   // the env's ints are drone 0's
        hipLaunchKernelGGL(spread_ints_kernel, dim3((h->E + 255) / 256), dim3(256), 0, s, h->ist, h->ni, h->E, h->N);
        HIPCHK(h, hipGetLastError());
    }
    return ADRP_OK;
}

// ---------------------------------------------------------------------------------------------
// roofline accounting: algorithmic HBM bytes of one adrp_step
// ---------------------------------------------------------------------------------------------
extern "C" int64_t adrp_step_bytes(const adrp_t* h) {
    if (!h) return ADRP_ERR_INVALID;
    if (h->cfg.task == ADRP_TASK_RACE) {
        // per drone: 64 state fields read + 60 written (mass/inertia are read-only), the env's
        // 28 track fields read, 9 ints read + 7 written, the FULLSTATE action, the obs row;
        // per env: reward + 2 flags (+ RewardWrapper: 6 fields r/w, 1 int)
        const int64_t rs = int64_t(h->real_size);
        const int64_t per_drone = (64 + 60 + 28) * rs + (9 + 7) * 4 + 16 + int64_t(h->D) * 4;
        const int64_t per_env = 6 + (h->cfg.track.reward_wrapper ? 12 * rs + 4 : 0);
        return (per_drone * h->N + per_env) * h->E;
    }
    const int ph = h->cfg.physics;
    const bool dyn = ph == ADRP_PHYS_DYN;
    const bool drag = ph == ADRP_PHYS_PYB_DRAG || ph == ADRP_PHYS_PYB_GND_DRAG_DW;
    const bool lag = h->cfg.link_frame_lag && !dyn;
    const int64_t fields = 13 + (lag ? 4 : 0) + (drag ? 4 : 0) + (dyn ? 3 : 0) + (h->nf_base - HF_NBASE);
    if (is_ctrl_task(h->cfg.task)) {
        // per drone: the state read and written (last_rpm read only by the drag modes, written by all),
        // step_counter read + written, the action (float32, or the handle's precision through
        // adrp_step_rpm: counted as float32), the 80-byte row; per env: reward + 2 flags
        const int64_t per_drone = (2 * fields + (drag ? 0 : 4)) * int64_t(h->real_size) + 2 * 4 + 4 * 4 + kCtrlObs * 4;
        return (per_drone * h->N + 6) * h->E;
    }
    const int64_t per_env = 2 * fields * int64_t(h->real_size)   // state read + write
                            + 2 * HI_N * 4                        // int state read + write
                            + int64_t(h->A) * 4                   // action
                            + int64_t(h->A) * 4                   // ring append
                            + int64_t(h->B - 1) * h->A * 4        // ring read
                            + int64_t(h->D) * 4                   // obs write
                            + 4 + 2;                              // reward, terminated, truncated
    if (h->cfg.task == ADRP_TASK_MULTIHOVER)   // per drone; reward and flags per env; the ring is read from HBM whole
        return ((per_env - 6 + int64_t(h->A) * 4) * h->N + 6) * h->E;
    return per_env * h->E;
}

// ---------------------------------------------------------------------------------------------
// persistent step (hover_persist.h): BASELINE config 1, one env stepped synchronously from Python
// ---------------------------------------------------------------------------------------------
static size_t a64(size_t n) { return (n + 63) & ~size_t(63); }

extern "C" int adrp_persistent_begin(adrp_t* h, void** act, void** obs, void** rew, void** term, void** trunc,
                                     void** tobs) {
    if (!h) return seterr(h, ADRP_ERR_INVALID, "adrp_persistent_begin: NULL handle");
    if (h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_persistent_begin: already active");
    if (h->cfg.task != ADRP_TASK_HOVER || hover_has_pid(h->cfg.act_type))
        return seterr(h, ADRP_ERR_INVALID, "adrp_persistent_begin: HoverAviary with RPM / ONE_D_RPM actions only");
    if (h->E > kPersistMaxBlocks * kStepBlock)
        return seterr(h, ADRP_ERR_INVALID, "adrp_persistent_begin: at most 1024 envs (one resident workgroup per 64)");
    DeviceGuard g(h->device);
    HIPCHK(h, hipDeviceSynchronize());   // every step / reset / set_state issued before is in the state
    const size_t E = size_t(h->E), D = size_t(h->D), A = size_t(h->A);
    // line mode (BASELINE config 1: E = 1): the actions and the request tag in one 64-byte line
    // (ADRP_PERSIST_LINE=0 keeps the request word + action rows form)
    const char* lm = getenv("ADRP_PERSIST_LINE");
    h->pline = E * A <= size_t(kPersistLineWords - 1) && !(lm && atoi(lm) == 0);
    size_t off = a64(sizeof(PersistCtl));
    const size_t sizes[6] = {h->pline ? size_t(4 * kPersistLineWords) : E * A * 4, E * D * 4, E * 4, E, E, E * D * 4};
    for (int k = 0; k < 6; ++k) {
        h->poff[k] = off;
        off += a64(sizes[k]);
    }
    void* box = nullptr;
    if (hipHostMalloc(&box, off, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return seterr(h, ADRP_ERR_OOM, "adrp_persistent_begin: hipHostMalloc");
    memset(box, 0, off);
    char* dbox = nullptr;
    if (hipHostGetDevicePointer((void**)&dbox, box, 0) != hipSuccess ||
        hipStreamCreateWithFlags(&h->pstream, hipStreamNonBlocking) != hipSuccess) {
        hipHostFree(box);
        h->pstream = nullptr;
        return seterr(h, ADRP_ERR_DEVICE, "adrp_persistent_begin: mapping / stream");
    }
    const int rc = h->real_size == 8 ? [&] {
        HoverArgs<double> a = hover_args<double>(h);
        a.act = (const float*)(dbox + h->poff[0]); a.obs = (float*)(dbox + h->poff[1]); a.rew = (float*)(dbox + h->poff[2]);
        a.term = (uint8_t*)(dbox + h->poff[3]); a.trunc = (uint8_t*)(dbox + h->poff[4]);
        a.tobs = h->cfg.autoreset ? (float*)(dbox + h->poff[5]) : nullptr;
        a.contact_count = nullptr;
        return hover_persist_launch<double>(h, a, dbox, h->pstream);
    }() : [&] {
        HoverArgs<float> a = hover_args<float>(h);
        a.act = (const float*)(dbox + h->poff[0]); a.obs = (float*)(dbox + h->poff[1]); a.rew = (float*)(dbox + h->poff[2]);
        a.term = (uint8_t*)(dbox + h->poff[3]); a.trunc = (uint8_t*)(dbox + h->poff[4]);
        a.tobs = h->cfg.autoreset ? (float*)(dbox + h->poff[5]) : nullptr;
        a.contact_count = nullptr;
        return hover_persist_launch<float>(h, a, dbox, h->pstream);
    }();
    if (rc != ADRP_OK) {
        hipStreamDestroy(h->pstream);
        h->pstream = nullptr;
        hipHostFree(box);
        return rc;
    }
    PersistCtl* ctl = (PersistCtl*)box;
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&ctl->status, __ATOMIC_ACQUIRE) != 1u) {   // resident before the first request
        if (hipStreamQuery(h->pstream) != hipErrorNotReady ||
            std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
            __atomic_store_n(&ctl->req, kPersistStop, __ATOMIC_RELEASE);
            hipStreamSynchronize(h->pstream);
            hipStreamDestroy(h->pstream);
            h->pstream = nullptr;
            hipHostFree(box);
            return seterr(h, ADRP_ERR_DEVICE, "adrp_persistent_begin: the persistent kernel did not start");
        }
    }
    h->pbox = box;
    h->pseq = 0;
    char* hb = (char*)box;
    if (act) *act = hb + h->poff[0];
    if (obs) *obs = hb + h->poff[1];
    if (rew) *rew = hb + h->poff[2];
    if (term) *term = hb + h->poff[3];
    if (trunc) *trunc = hb + h->poff[4];
    if (tobs) *tobs = hb + h->poff[5];
    return ADRP_OK;
}

extern "C" int adrp_persistent_step(adrp_t* h) {
    if (!h || !h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_persistent_step: persistent mode is not active");
    PersistCtl* ctl = (PersistCtl*)h->pbox;
    if (__atomic_load_n(&ctl->kstop, __ATOMIC_ACQUIRE) != 0u || __atomic_load_n(&ctl->status, __ATOMIC_ACQUIRE) == 2u)
        return seterr(h, ADRP_ERR_DEVICE, "adrp_persistent_step: the persistent kernel has exited "
                                          "(idle timeout); adrp_persistent_end, then begin again");
    uint32_t seq = h->pseq + 1;
    if (seq == kPersistStop) seq = 1;
    h->pseq = seq;
    // the action bytes written before it are visible first (x86 stores are not reordered; release)
    if (h->pline) __atomic_store_n((uint32_t*)((char*)h->pbox + h->poff[0]) + (kPersistLineWords - 1), seq, __ATOMIC_RELEASE);
    else __atomic_store_n(&ctl->req, seq, __ATOMIC_RELEASE);
    const int nb = (h->E + kStepBlock - 1) / kStepBlock;
    for (int b = 0; b < nb; ++b) {
        unsigned spins = 0;
        auto t0 = std::chrono::steady_clock::time_point{};
        while (__atomic_load_n(&ctl->done[b], __ATOMIC_ACQUIRE) != seq) {
            __builtin_ia32_pause();
            if ((++spins & 4095u) == 0) {
                if (t0 == decltype(t0){}) t0 = std::chrono::steady_clock::now();
                // workgroup b left on the grid-wide idle timeout without this request: the step
                // may have run on the other workgroups' envs only
                if (__atomic_load_n(&ctl->exited[b], __ATOMIC_ACQUIRE) != 0u &&
                    __atomic_load_n(&ctl->done[b], __ATOMIC_ACQUIRE) != seq)
                    return seterr(h, ADRP_ERR_DEVICE, "adrp_persistent_step: the persistent kernel has exited "
                                                      "(idle timeout) before completing this step, whose envs may "
                                                      "be partially stepped; adrp_persistent_end, then begin again");
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
                    return seterr(h, ADRP_ERR_DEVICE, "adrp_persistent_step: no completion within 10 s");
            }
        }
    }
    return ADRP_OK;
}

extern "C" int adrp_persistent_end(adrp_t* h) {
    if (!h || !h->pbox) return seterr(h, ADRP_ERR_INVALID, "adrp_persistent_end: persistent mode is not active");
    DeviceGuard g(h->device);
    PersistCtl* ctl = (PersistCtl*)h->pbox;
    __atomic_store_n(&ctl->req, kPersistStop, __ATOMIC_RELEASE);
    if (h->pline) __atomic_store_n((uint32_t*)((char*)h->pbox + h->poff[0]) + (kPersistLineWords - 1), kPersistStop, __ATOMIC_RELEASE);
    const hipError_t e = hipStreamSynchronize(h->pstream);
    hipStreamDestroy(h->pstream);
    hipHostFree(h->pbox);
    h->pstream = nullptr;
    h->pbox = nullptr;
    if (e != hipSuccess) return seterr(h, ADRP_ERR_DEVICE, std::string("adrp_persistent_end: ") + hipGetErrorString(e));
    return ADRP_OK;
}

// ---------------------------------------------------------------------------------------------
// kernel timing and diagnostics
// ---------------------------------------------------------------------------------------------
extern "C" int adrp_profile_begin(adrp_t* h, int max_launches) {
    if (!h || max_launches < 0 || max_launches > (1 << 20)) return seterr(h, ADRP_ERR_INVALID, "max_launches");
    DeviceGuard g(h->device);
    while ((int)h->ev_start.size() < max_launches) {
        hipEvent_t a, b;
        HIPCHK(h, hipEventCreate(&a));
        HIPCHK(h, hipEventCreate(&b));
        h->ev_start.push_back(a);
        h->ev_stop.push_back(b);
    }
    h->prof_cap = max_launches;
    h->prof_n = 0;
    return ADRP_OK;
}

extern "C" int adrp_profile_end(adrp_t* h, float* kernel_ms, int cap) {
    if (!h) return ADRP_ERR_INVALID;
    DeviceGuard g(h->device);
    const int n = std::min(h->prof_n, cap);
    for (int k = 0; k < n; ++k) {
        HIPCHK(h, hipEventSynchronize(h->ev_stop[k]));
        HIPCHK(h, hipEventElapsedTime(&kernel_ms[k], h->ev_start[k], h->ev_stop[k]));
    }
    h->prof_cap = 0;
    h->prof_n = 0;
    return n;
}

extern "C" int adrp_set_diagnostics(adrp_t* h, int enable) {
    if (!h) return ADRP_ERR_INVALID;
    if (enable && h->cfg.task == ADRP_TASK_RACE && !h->mom_hash) {
        DeviceGuard g(h->device);
        const size_t bytes = size_t(h->E) * h->N * sizeof(uint32_t);
        if (hipMalloc((void**)&h->mom_hash, bytes) != hipSuccess) {
            h->mom_hash = nullptr;
            return seterr(h, ADRP_ERR_OOM, "adrp_set_diagnostics: hipMalloc failed");
        }
        if (hipMemset(h->mom_hash, 0, bytes) != hipSuccess) return seterr(h, ADRP_ERR_DEVICE, "adrp_set_diagnostics");
    }
    if (enable >= 2 && h->cfg.task == ADRP_TASK_RACE && !h->mom_log) {
        DeviceGuard g(h->device);
        const size_t EN = size_t(h->E) * h->N;
        if (hipMalloc((void**)&h->mom_log, EN * size_t(h->S) * 3 * sizeof(int16_t)) != hipSuccess ||
            hipMalloc((void**)&h->mom_log_n, EN * sizeof(int32_t)) != hipSuccess)
            return seterr(h, ADRP_ERR_OOM, "adrp_set_diagnostics: hipMalloc failed (moment log)");
        if (hipMemset(h->mom_log_n, 0, EN * sizeof(int32_t)) != hipSuccess)
            return seterr(h, ADRP_ERR_DEVICE, "adrp_set_diagnostics");
    }
    h->diagnostics = enable >= 2 && h->cfg.task == ADRP_TASK_RACE ? 2 : enable ? 1 : 0;
    return ADRP_OK;
}

// race diagnostics level 2: the int16 (roll, pitch, yaw) moments of every firmware call of the last
// env.step, per drone in call order, and the number of calls (the one-lane kernel records them)
extern "C" int adrp_race_moment_log(adrp_t* h, int16_t* out, int32_t* counts, size_t n, int max_calls) {
    if (!h || !out || !counts) return seterr(h, ADRP_ERR_INVALID, "adrp_race_moment_log: NULL argument");
    if (h->cfg.task != ADRP_TASK_RACE || !h->mom_log || h->diagnostics < 2)
        return seterr(h, ADRP_ERR_INVALID, "adrp_race_moment_log: a race handle with diagnostics level 2");
    if (n != size_t(h->E) * h->N || max_calls != h->S)
        return seterr(h, ADRP_ERR_INVALID, "adrp_race_moment_log: n != E * N or max_calls != sub-steps");
    DeviceGuard g(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out, h->mom_log, n * size_t(max_calls) * 3 * sizeof(int16_t), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(counts, h->mom_log_n, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ADRP_OK;
}

// race diagnostics: the per-drone hash of the int16 firmware moments of the last env.step
// (race_kernel.h fw_moment_hash), copied to host memory after the handle's device finishes
extern "C" int adrp_race_moment_hash(adrp_t* h, uint32_t* out, size_t n) {
    if (!h || !out) return seterr(h, ADRP_ERR_INVALID, "adrp_race_moment_hash: NULL argument");
    if (h->cfg.task != ADRP_TASK_RACE || !h->mom_hash)
        return seterr(h, ADRP_ERR_INVALID, "adrp_race_moment_hash: a race handle with diagnostics on");
    if (n != size_t(h->E) * h->N) return seterr(h, ADRP_ERR_INVALID, "adrp_race_moment_hash: n != E * N");
    DeviceGuard g(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out, h->mom_hash, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ADRP_OK;
}

#ifdef ADRP_RACE_TIMING
// timing build only (not declared in include/adrp.h): per-phase s_memtime sums of the step
// kernels -- race: [setup, physics, controller, rays, obs, contacts, tail, total, waves, -]
// sums over waves, the same phases' max over waves at [10..17], GJK calls/iterations at
// 9/18/19; hover: tools/hover_phases.py.  Summed over the kernel code objects.
extern "C" int adrp_race_phase_read(unsigned long long* out, int reset) {
    int (*readers[8])(unsigned long long*, int) = {phase_read_hover_f32, phase_read_hover_f64, phase_read_race_f32,
                                                  phase_read_race_f32b, phase_read_race_f32c, phase_read_race_f64,
                                                  phase_read_race_f64b, phase_read_race_f64c};
    for (int k = 0; k < 32; ++k) out[k] = 0;
    for (auto rd : readers) {
        unsigned long long v[32];
        const int rc = rd(v, reset);
        if (rc != ADRP_OK) return rc;
        for (int k = 0; k < 32; ++k) {
            const bool is_max = (k >= 10 && k <= 17) || k == 19 || k == 21;
            out[k] = is_max ? std::max(out[k], v[k]) : out[k] + v[k];
        }
    }
    return ADRP_OK;
}
// per-workgroup phases of the fp32 four-lane race kernel: n slots of [setup, physics, controller,
// rays, obs, contacts, tail, total] s_memtime cycles (RACE_WAVE), written by the last launch
extern "C" int adrp_race_wave_read(unsigned long long* out, int n) { return wave_read_race_f32(out, n); }
extern "C" int adrp_race_wave_read_f64(unsigned long long* out, int n) { return wave_read_race_f64(out, n); }
#ifdef ADRP_RACE_GJK_STATS
// capped GJK queries of the PYB / PYB_DW race kernels (race_f32.hip / race_f64.hip code objects):
// up to `max` records of kGjkDumpF doubles; returns the count copied (-1 on error)
extern "C" int adrp_gjk_dump_read(double* out, int max, int f64, int reset) {
    return f64 ? gjk_dump_read_f64(out, max, reset) : gjk_dump_read_f32(out, max, reset);
}
#endif
#endif

extern "C" int adrp_race_reset_counts(adrp_t* h, int32_t* out, int reset) {
    if (!h || !out) return seterr(h, ADRP_ERR_INVALID, "adrp_race_reset_counts: NULL argument");
    DeviceGuard g(h->device);
    HIPCHK(h, hipMemcpy(out, h->counters + 1, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(h, hipMemset(h->counters + 1, 0, 2 * sizeof(int32_t)));
    return ADRP_OK;
}

extern "C" int adrp_diagnostic_contact_count(adrp_t* h, int reset) {
    if (!h) return ADRP_ERR_INVALID;
    DeviceGuard g(h->device);
    int32_t v = 0;
    if (hipMemcpy(&v, h->counters, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return ADRP_ERR_DEVICE;
    if (reset && hipMemset(h->counters, 0, sizeof(int32_t)) != hipSuccess) return ADRP_ERR_DEVICE;
    return v;
}
