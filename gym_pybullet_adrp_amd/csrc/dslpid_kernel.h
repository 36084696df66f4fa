// dslpid_kernel.h — stand-alone batched DSLPIDControl for gfx950: one lane per controller row (one
// (env, drone) pair, rows = E * N), one launch per computeControl call.
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   DSLPIDControl.computeControl        control/DSLPIDControl.py:82-145
//   _dslPIDPositionControl              control/DSLPIDControl.py:149-208
//   _dslPIDAttitudeControl              control/DSLPIDControl.py:212-259
//   BaseControl.computeControlFromState control/BaseControl.py:55-95 (state[0:3], [3:7], [10:13])
//
// The position and attitude loops are dslpid_core.h's, the one copy that dslpid_rpm (hover_dynamics.h), the
// controller fused into the HoverAviary / VelocityAviary step kernels, calls too.  That one has the
// targets of its action types, the default gains and the CF2X mixer compiled in; here the four targets,
// the gains, the mixer and control_timestep are runtime values, and pos_e and the yaw error are returned.
// tests/test_dslpid_gpu.py compares the two callers.
//
// The yaw error is computed_target_rpy[2] - cur_rpy[2] (:145): the first is the THIRD angle of scipy's
// intrinsic 'XYZ' decomposition of the target basis T = [x y z] = Rx(a) Ry(b) Rz(c) (:205), i.e.
// c = atan2(-T01, T00) = atan2(-y_ax.x, x_ax.x), not the yaw of the extrinsic-xyz euler_xyz; the second
// is getEulerFromQuaternion's yaw (euler_xyz).
//
// Inputs come through (base pointer, component stride, row stride) per group, so one body serves state
// rows [rows][20], separate pos / quat / vel arrays and the SoA columns of an env handle.  Input elements
// may be float while the controller is double (converted on load).  Controller state is SoA [9][rows]:
// last_rpy 3, integral_pos_e 3, integral_rpy_e 3 (control/DSLPIDControl.py:65-79).
//
// Shape: a workgroup is one wave of 64 rows (kStepBlock: 4096 rows spread over 64 CUs); no LDS, barrier,
// atomic or cross-lane move; lanes past `rows` return before any load.
#pragma once

#include "adrp_device.h"
#include "dslpid_core.h"

namespace adrp {

constexpr int kDslpidBlock = 64;
constexpr int kDslpidState = 9;

// runtime constants of one call (setPIDCoefficients, the model's mixer, control_timestep)
template <typename Real>
struct DslpidConst {
    Real p_for[3], i_for[3], d_for[3], p_tor[3], i_tor[3], d_tor[3];
    Real mix[4][3];
    Real grav, inv4kf;                       // GRAVITY = g m, 1 / (4 KF)
    Real rpm_scale, rpm_const, inv_scale;    // PWM2RPM_SCALE, PWM2RPM_CONST, 1 / PWM2RPM_SCALE
    Real min_pwm, max_pwm;
    Real dt, hz;                             // control_timestep and its inverse
};

// one input group: component c of row r is p[r * rs + c * cs]
template <typename T>
struct DslpidVec {
    const T* p;
    long long cs, rs;
};

template <typename Real, typename TIn>
struct DslpidArgs {
    DslpidConst<Real> k;
    DslpidVec<TIn> pos, quat, vel;
    const Real* t_pos;     // [rows][3] each, or null = zeros
    const Real* t_rpy;
    const Real* t_vel;
    const Real* t_rates;
    Real* st;              // [9][rows], in / out
    Real* rpm;             // [rows][4]
    Real* pos_e;           // [rows][3] or null
    Real* yaw_e;           // [rows] or null
    int rows;
};

// computed_target_rpy[2] - cur_rpy[2] (:145): c = atan2(-y_ax.x, x_ax.x) minus getEulerFromQuaternion's yaw.
// It is a difference of two angles of order one that goes to zero as the drone reaches its yaw target, so in
// float32 the two roundings of the angles (1.2e-7 apart near 1 rad) would be all that is left of it.  The
// float32 kernel therefore evaluates both angles and their difference in float64 from its float32 operands
// (their products are exact there) and rounds once: the yaw straight from the quaternion, and c from the
// unnormalised thrust vector t and the yaw target, with y_c = z x (cy, sy, 0), x = y x z and z = t / |t|:
//   -y_ax.x |y_c| |t|^2 = t.z sy |t|,   x_ax.x |y_c| |t|^2 = t.z^2 cy - t.x t.y sy + t.y^2 cy
// (positive factors, which atan2 ignores), with the float64 fast forms of adrp_device.h (octant-reduced sincos,
// polynomial atan2: within an ulp of libm, far below the one float32 rounding that follows).  The float64
// kernel keeps the direct form.
template <typename Real>
__device__ __forceinline__ Real yaw_error(const Real tt[3], Real tyaw, Q4<Real> q, V3<Real> xax, V3<Real> yax, Real yaw) {
    if constexpr (sizeof(Real) == 8) {
        return atan2_(-yax.x, xax.x) - yaw;
    } else {
        const double tx = tt[0], ty = tt[1], tz = tt[2];
        double sy, cy;
        sincos_f_(double(tyaw), &sy, &cy);
        const double c = fatan2_(tz * sy * sqrt_(tx * tx + ty * ty + tz * tz), tz * tz * cy - tx * ty * sy + ty * ty * cy);
        const Q4<double> qd = {double(q.x), double(q.y), double(q.z), double(q.w)};
        return Real(c - euler_xyz_fast(qd).z);
    }
}

// computeControl of one row.  ctl = last_rpy 3, integral_pos_e 3, integral_rpy_e 3 (in / out); without want_yaw_e the yaw
// error is not evaluated (the float32 kernel skips its float64 part)
template <typename Real>
__device__ __forceinline__ void dslpid_control(const DslpidConst<Real>& K, V3<Real> pos, Q4<Real> q, V3<Real> vel,
                                               const Real tp[3], Real tyaw, const Real tv[3], const Real rates[3],
                                               Real ctl[kDslpidState], Real rpm[4], Real pos_e[3], bool want_yaw_e, Real& yaw_e) {
    const M3<Real> R = rot(q);
    const V3<Real> rpy = euler_xyz(q);
    Real thrust, tq[3], tt[3];
    V3<Real> xax, yax;
    dslpid_core<Real>(K, K.dt, K.hz, K.grav, K.inv4kf, K.rpm_const, K.inv_scale, R, rpy, pos, vel, tp, tyaw, tv, rates, ctl,
                      thrust, tq, pos_e, tt, xax, yax);
    if (want_yaw_e) yaw_e = yaw_error<Real>(tt, tyaw, q, xax, yax, rpy.z);   // (wave-uniform: the caller's pointer)
    // pwm = thrust + MIXER_MATRIX . torques, clipped, PWM -> RPM
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Real mixed = K.mix[i][0] * tq[0] + K.mix[i][1] * tq[1] + K.mix[i][2] * tq[2];
        rpm[i] = K.rpm_scale * clip_(thrust + mixed, K.min_pwm, K.max_pwm) + K.rpm_const;
    }
}

template <typename Real, typename TIn>
__global__ __launch_bounds__(kDslpidBlock) void dslpid_control_kernel(const DslpidArgs<Real, TIn> a) {
    const int r = blockIdx.x * kDslpidBlock + threadIdx.x;
    if (r >= a.rows) return;
    const long long rr = r;
    const size_t rows = size_t(a.rows);
    const TIn* pp = a.pos.p + rr * a.pos.rs;
    const TIn* qp = a.quat.p + rr * a.quat.rs;
    const TIn* vp = a.vel.p + rr * a.vel.rs;
    const V3<Real> pos = v3(Real(pp[0]), Real(pp[a.pos.cs]), Real(pp[2 * a.pos.cs]));
    const Q4<Real> q = {Real(qp[0]), Real(qp[a.quat.cs]), Real(qp[2 * a.quat.cs]), Real(qp[3 * a.quat.cs])};
    const V3<Real> vel = v3(Real(vp[0]), Real(vp[a.vel.cs]), Real(vp[2 * a.vel.cs]));
    Real tp[3] = {Real(0), Real(0), Real(0)}, tv[3] = {Real(0), Real(0), Real(0)}, rates[3] = {Real(0), Real(0), Real(0)};
    Real tyaw = Real(0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (a.t_pos) tp[k] = a.t_pos[rr * 3 + k];
        if (a.t_vel) tv[k] = a.t_vel[rr * 3 + k];
        if (a.t_rates) rates[k] = a.t_rates[rr * 3 + k];
    }
    if (a.t_rpy) tyaw = a.t_rpy[rr * 3 + 2];    // (only the yaw target enters, :200)
    Real ctl[kDslpidState];
#pragma unroll
    for (int k = 0; k < kDslpidState; ++k) ctl[k] = a.st[k * rows + r];
    Real rpm[4], pos_e[3], yaw_e = Real(0);
    dslpid_control<Real>(a.k, pos, q, vel, tp, tyaw, tv, rates, ctl, rpm, pos_e, a.yaw_e != nullptr, yaw_e);
#pragma unroll
    for (int k = 0; k < kDslpidState; ++k) a.st[k * rows + r] = ctl[k];
#pragma unroll
    for (int i = 0; i < 4; ++i) a.rpm[rr * 4 + i] = rpm[i];
    if (a.pos_e) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.pos_e[rr * 3 + k] = pos_e[k];
    }
    if (a.yaw_e) a.yaw_e[r] = yaw_e;
}

// reset(): zero the nine state values of the rows with mask[r] != 0
template <typename Real>
__global__ void dslpid_reset_kernel(Real* st, const uint8_t* mask, int rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows || !mask[r]) return;
#pragma unroll
    for (int k = 0; k < kDslpidState; ++k) st[size_t(k) * rows + r] = Real(0);
}

}  // namespace adrp
