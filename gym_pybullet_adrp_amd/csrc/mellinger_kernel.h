// mellinger_kernel.h — stand-alone batched MellingerControl for gfx950: one lane per controller row (one
// (env, drone) pair, rows = E * N), one launch per computeControl call.
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   MellingerControl.reset           control/MellingerControl.py:99-150
//   MellingerControl.computeControl  control/MellingerControl.py:154-262
//   low_level_control                control/MellingerControl.py:17-61 (send*Cmd, process_command_queue)
//
// Nothing of the controller is restated here: the wrapper arithmetic, the tick schedule, the tumble check,
// the firmware, its filters and the PWM chain are race_kernel.h's mellinger_compute<Real, CMD = true> (with
// mellinger_fw, lpf_apply, tick_window), the commander is commander.h's hl_* — the functions the fused
// race step kernels call once per 500 Hz sub-step.  This header only moves one row's state between memory
// and the RDrone / CmdState registers those functions work on, so a test of this kernel at a constructed
// controller state is a test of the race kernels' controller (tests/test_mellinger_gpu.py).
//
// The body rotation: the reference hands the firmware get_quaternion_from_euler(cur_rpy); the race kernels
// pass the body quaternion itself.  Here the caller gives roll / pitch / yaw (or, for an env handle, the
// kernel takes them from the quaternion column with euler_xyz_fast_u, the race kernels' controller input),
// and the quaternion mellinger_compute reads is quat_from_euler_fast of those angles.
//
// Inputs come through (base pointer, component stride, row stride) per group, as in dslpid_kernel.h.
// Controller state is SoA: Real [MF_N][rows] (the oracle's field names, mellinger.hip k_mell_f),
// int32 [MI_N][rows], and the command state float [ADRP_CMD_NF][rows] + int32 [ADRP_CMD_NI][rows]
// (commander.h), so a wave's loads and stores coalesce.
//
// Shape: a workgroup is one wave of 64 rows; no LDS, barrier or atomic; lanes past `rows` return before any
// load (the wave votes inside mellinger_compute / tick_window count active lanes only).
#pragma once

#include "race_kernel.h"

namespace adrp {

constexpr int kMellBlock = 64;

// float fields, in the order of the oracle's race state (oracle/race.c race_field_name)
enum MellField {
    MF_RPM = 0, MF_PREV_RPM = 4, MF_PREV_RPY = 8, MF_PREV_VEL = 11, MF_LPF_D1 = 14, MF_LPF_D2 = 17, MF_I_ERR = 20,
    MF_I_ERR_M = 23, MF_PREV_OMEGA_ROLL = 26, MF_PREV_OMEGA_PITCH = 27, MF_PREV_SP_ROLL = 28, MF_PREV_SP_PITCH = 29,
    MF_CTL = 30, MF_N = 34
};
enum MellInt { MI_TICK = 0, MI_LAST_ATT, MI_LAST_POS, MI_TUMBLE, MI_N };

// one input group: component c of row r is p[r * rs + c * cs]
template <typename T>
struct MellVec {
    const T* p;
    long long cs, rs;
};

template <typename Real, typename TIn>
struct MellArgs {
    MellVec<TIn> pos, ang, vel;   // ang: roll / pitch / yaw, or (ENV) the quaternion xyzw
    const Real* noise;            // [rows][4] thrust disturbance, or null = zeros
    Real* st;                     // [MF_N][rows]
    int32_t* ist;                 // [MI_N][rows]
    float* cf;                    // [ADRP_CMD_NF][rows]
    int32_t* ci;                  // [ADRP_CMD_NI][rows]
    const uint32_t* ticks;        // race_tick_tables: att [kTickWords], pos [kTickWords]
    Real* rpm;                    // [rows][4]
    Real* rpy_out;                // [rows][3] the angles the controller was fed, or null
    const uint8_t* mask;          // reset: rows to reset, or null = all
    const int32_t* cmd;           // command: [rows] ADRP_CMD_*
    const double* cargs;          // command: [rows][ADRP_CMD_ARGS]
    Lpf lpf;                      // lpf2pInit(gyrolpf, 500, 30), host float
    int rows;
};

template <typename Real>
__device__ __forceinline__ void mell_load(const Real* st, const int32_t* ist, size_t rows, size_t r, RDrone<Real>& d) {
#define L_(k) st[size_t(k) * rows + r]
#pragma unroll
    for (int k = 0; k < 4; ++k) { d.rpm[k] = L_(MF_RPM + k); d.prev[k] = L_(MF_PREV_RPM + k); d.ctl[k] = float(L_(MF_CTL + k)); }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d.prev_rpy[k] = L_(MF_PREV_RPY + k); d.prev_vel[k] = L_(MF_PREV_VEL + k);
        d.lpf1[k] = float(L_(MF_LPF_D1 + k)); d.lpf2[k] = float(L_(MF_LPF_D2 + k));
        d.ierr[k] = float(L_(MF_I_ERR + k)); d.ierrm[k] = float(L_(MF_I_ERR_M + k));
    }
    d.pw_roll = float(L_(MF_PREV_OMEGA_ROLL)); d.pw_pitch = float(L_(MF_PREV_OMEGA_PITCH));
    d.psp_roll = float(L_(MF_PREV_SP_ROLL)); d.psp_pitch = float(L_(MF_PREV_SP_PITCH));
#undef L_
    d.tick = ist[MI_TICK * rows + r]; d.last_att = ist[MI_LAST_ATT * rows + r];
    d.last_pos = ist[MI_LAST_POS * rows + r]; d.tumble = ist[MI_TUMBLE * rows + r];
}

template <typename Real>
__device__ __forceinline__ void mell_store(Real* st, int32_t* ist, size_t rows, size_t r, const RDrone<Real>& d) {
#define S_(k, v) st[size_t(k) * rows + r] = Real(v)
#pragma unroll
    for (int k = 0; k < 4; ++k) { S_(MF_RPM + k, d.rpm[k]); S_(MF_PREV_RPM + k, d.prev[k]); S_(MF_CTL + k, d.ctl[k]); }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        S_(MF_PREV_RPY + k, d.prev_rpy[k]); S_(MF_PREV_VEL + k, d.prev_vel[k]);
        S_(MF_LPF_D1 + k, d.lpf1[k]); S_(MF_LPF_D2 + k, d.lpf2[k]);
        S_(MF_I_ERR + k, d.ierr[k]); S_(MF_I_ERR_M + k, d.ierrm[k]);
    }
    S_(MF_PREV_OMEGA_ROLL, d.pw_roll); S_(MF_PREV_OMEGA_PITCH, d.pw_pitch);
    S_(MF_PREV_SP_ROLL, d.psp_roll); S_(MF_PREV_SP_PITCH, d.psp_pitch);
#undef S_
    ist[MI_TICK * rows + r] = d.tick; ist[MI_LAST_ATT * rows + r] = d.last_att;
    ist[MI_LAST_POS * rows + r] = d.last_pos; ist[MI_TUMBLE * rows + r] = d.tumble;
}

// one MellingerControl.computeControl call per row
template <typename Real, typename TIn, bool ENV>
__global__ __launch_bounds__(kMellBlock) void mellinger_compute_kernel(const MellArgs<Real, TIn> a) {
    const int r = blockIdx.x * kMellBlock + threadIdx.x;
    if (r >= a.rows) return;
    const long long rr = r;
    const size_t rows = size_t(a.rows);
    const TIn* pp = a.pos.p + rr * a.pos.rs;
    const TIn* ap = a.ang.p + rr * a.ang.rs;
    const TIn* vp = a.vel.p + rr * a.vel.rs;
    RDrone<Real> d;
    d.pos = v3(Real(pp[0]), Real(pp[a.pos.cs]), Real(pp[2 * a.pos.cs]));
    d.vel = v3(Real(vp[0]), Real(vp[a.vel.cs]), Real(vp[2 * a.vel.cs]));
    V3<Real> rpy;
    if constexpr (ENV) {
        const Q4<Real> qb = {Real(ap[0]), Real(ap[a.ang.cs]), Real(ap[2 * a.ang.cs]), Real(ap[3 * a.ang.cs])};
        rpy = euler_xyz_fast_u(qb);
    } else {
        rpy = v3(Real(ap[0]), Real(ap[a.ang.cs]), Real(ap[2 * a.ang.cs]));
    }
    d.q = quat_from_euler_fast(rpy.x, rpy.y, rpy.z);
    Real noise[4] = {Real(0), Real(0), Real(0), Real(0)};
    if (a.noise) {
#pragma unroll
        for (int k = 0; k < 4; ++k) noise[k] = a.noise[rr * 4 + k];
    }
    mell_load(a.st, a.ist, rows, size_t(r), d);
    if (d.tick < 0) d.tick = 0;   // (a tick is a count of calls; a negative one from set_state counts as 0)
    d.tick_base = d.tick;
    tick_window(a.ticks, d.tick, d.att_bits, d.pos_bits);
    d.mh = kMomHashSeed;
    CmdState cs;
    cmd_load(a.cf, a.ci, rows, size_t(r), cs);
    const float sp[3] = {0.0f, 0.0f, 0.0f};   // (unused with CMD: the setpoint is the command state's)
    mellinger_compute<Real, true>(d, a.lpf, sp, 0.0f, 0.0f, rpy, noise, &cs, a.cf + size_t(CF_COEF) * rows, rows,
                                  size_t(r));
    mell_store(a.st, a.ist, rows, size_t(r), d);
    cmd_store(a.cf, a.ci, rows, size_t(r), cs);
#pragma unroll
    for (int k = 0; k < 4; ++k) a.rpm[rr * 4 + k] = d.rpm[k];
    if (a.rpy_out) {
        a.rpy_out[rr * 3] = rpy.x; a.rpy_out[rr * 3 + 1] = rpy.y; a.rpy_out[rr * 3 + 2] = rpy.z;
    }
}

// MellingerControl.reset(init_obs) of the rows with mask[r] != 0 (all without a mask): what race_reset_lane
// does for the controller part of a drone, with the caller's pose for the nominal one
template <typename Real, typename TIn>
__global__ __launch_bounds__(kMellBlock) void mellinger_reset_kernel(const MellArgs<Real, TIn> a) {
    const int r = blockIdx.x * kMellBlock + threadIdx.x;
    if (r >= a.rows || (a.mask && !a.mask[r])) return;
    const long long rr = r;
    const size_t rows = size_t(a.rows);
    const TIn* pp = a.pos.p + rr * a.pos.rs;
    const TIn* ap = a.ang.p + rr * a.ang.rs;
    const TIn* vp = a.vel.p + rr * a.vel.rs;
    RDrone<Real> d;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d.prev_rpy[k] = Real(ap[k * a.ang.cs]); d.prev_vel[k] = Real(vp[k * a.vel.cs]);
        d.lpf1[k] = d.lpf2[k] = 0.0f; d.ierr[k] = d.ierrm[k] = 0.0f;
    }
    d.tick = d.last_att = d.last_pos = d.tumble = 0;
    d.pw_roll = d.pw_pitch = __builtin_nanf("");   // the first firmware call has no D term
    d.psp_roll = d.psp_pitch = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { d.ctl[k] = 0.0f; d.rpm[k] = d.prev[k] = Real(0); }
    mell_store(a.st, a.ist, rows, size_t(r), d);
    CmdState cs;
    hl_reset(cs, float(Real(pp[0])), float(Real(pp[a.pos.cs])), float(Real(pp[2 * a.pos.cs])),
             float(d.prev_rpy[2] * Real(57.29577951308232)));
    cmd_store(a.cf, a.ci, rows, size_t(r), cs);
    for (int k = 0; k < 32; ++k) a.cf[size_t(CF_COEF + k) * rows + r] = 0.0f;
}

// one command message per row (low_level_control: send*Cmd, then process_command_queue(args[-1]))
template <typename Real, typename TIn>
__global__ __launch_bounds__(kMellBlock) void mellinger_command_kernel(const MellArgs<Real, TIn> a) {
    const int r = blockIdx.x * kMellBlock + threadIdx.x;
    if (r >= a.rows) return;
    const size_t rows = size_t(a.rows);
    const int code = a.cmd[r];
    if (code <= ADRP_CMD_NONE || code > ADRP_CMD_NOTIFY) return;
    CmdState cs;
    cmd_load(a.cf, a.ci, rows, size_t(r), cs);
    hl_command(cs, a.cf + size_t(CF_COEF) * rows, rows, size_t(r), code, a.cargs + size_t(r) * ADRP_CMD_ARGS, false);
    cmd_store(a.cf, a.ci, rows, size_t(r), cs);
}

}  // namespace adrp
