// dslpid_core.h — the one copy of DSLPIDControl's two loops for gfx950, shared by the controller fused
// into the HoverAviary / VelocityAviary step kernels (dslpid_rpm, hover_dynamics.h) and the stand-alone
// batched controller (dslpid_control, dslpid_kernel.h).
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   _dslPIDPositionControl              control/DSLPIDControl.py:149-208
//   _dslPIDAttitudeControl              control/DSLPIDControl.py:212-259
//
// The callers keep what differs between them: how the four targets are chosen, and the mixer with the
// PWM -> RPM step (literal CF2X sums in the fused controller, a runtime 4 x 3 matrix in the stand-alone
// one: merging them would change the fused controller's rounding).  Conventions: the scipy Euler round
// trip of the target rotation (:205, :242-244) is the identity on a proper rotation, so the target basis
// is used directly; the clips are compare-selects; the current Euler angles are the caller's, from the
// accurate conversion (the attitude D term scales their error by D_COEFF_TOR / control_timestep, about
// 1e6 at 48 Hz).
#pragma once

#include "adrp_device.h"

namespace adrp {

template <typename Real>
__device__ __forceinline__ Real clip_(Real x, Real lo, Real hi) {
    return x < lo ? lo : (x > hi ? hi : x);
}

// the six gain vectors of DSLPIDControl (P / I / D_COEFF_FOR, P / I / D_COEFF_TOR) on their own
template <typename Real>
struct DslpidGains {
    Real p_for[3], i_for[3], d_for[3], p_tor[3], i_tor[3], d_tor[3];
};

// K: the gains, any type with p_for, i_for, d_for, p_tor, i_tor, d_tor [3] each.  dt, hz: control_timestep
// and its inverse; grav = g m; inv4kf = 1 / (4 KF); rpm_const, inv_scale: PWM2RPM_CONST, 1 / PWM2RPM_SCALE.
// R = rot(q) and rpy = euler_xyz(q) come from the caller, who needs them too (the accurate conversion
// holds wave votes, so two calls are not merged).  ctl = last_rpy 3, integral_pos_e 3, integral_rpy_e 3
// (in / out).  Out: the scalar thrust (PWM), the clipped target torques tq, pos_e, and the target
// thrust vector tt with the target basis' x and y axes (the stand-alone controller's yaw error).
template <typename Real, typename Gains>
__device__ __forceinline__ void dslpid_core(const Gains& K, Real dt, Real hz, Real grav, Real inv4kf, Real rpm_const,
                                            Real inv_scale, const M3<Real>& R, V3<Real> rpy, V3<Real> pos, V3<Real> vel,
                                            const Real tp[3], Real tyaw, const Real tv[3], const Real rates[3],
                                            Real ctl[9], Real& thrust, Real tq[3], Real pos_e[3], Real tt[3],
                                            V3<Real>& xax, V3<Real>& yax) {
    // _dslPIDPositionControl (:149-208)
    const Real cp[3] = {pos.x, pos.y, pos.z}, cv[3] = {vel.x, vel.y, vel.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const Real pe = tp[k] - cp[k], ve = tv[k] - cv[k];
        pos_e[k] = pe;
        Real ip = clip_(ctl[3 + k] + pe * dt, Real(-2), Real(2));
        if (k == 2) ip = clip_(ip, Real(-0.15), Real(0.15));
        ctl[3 + k] = ip;
        tt[k] = K.p_for[k] * pe + K.i_for[k] * ip + K.d_for[k] * ve;
    }
    tt[2] += grav;
    Real sc = tt[0] * R.a02 + tt[1] * R.a12 + tt[2] * R.a22;
    sc = sc < Real(0) ? Real(0) : sc;
    thrust = (sqrt_(sc * inv4kf) - rpm_const) * inv_scale;
    const V3<Real> ttv = v3(tt[0], tt[1], tt[2]);
    const V3<Real> zax = rsqrt_(dot(ttv, ttv)) * ttv;
    Real sy, cy;
    sincos_(tyaw, &sy, &cy);
    const V3<Real> yc = cross(zax, v3(cy, sy, Real(0)));
    yax = rsqrt_(dot(yc, yc)) * yc;
    xax = cross(yax, zax);
    // _dslPIDAttitudeControl (:212-259): rot_e = vee(Rt^T R - R^T Rt)
    const V3<Real> c0 = v3(R.a00, R.a10, R.a20), c1 = v3(R.a01, R.a11, R.a21), c2 = v3(R.a02, R.a12, R.a22);
    const Real rot_e[3] = {dot(zax, c1) - dot(c2, yax), dot(xax, c2) - dot(c0, zax), dot(yax, c0) - dot(c1, xax)};
    const Real cur[3] = {rpy.x, rpy.y, rpy.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const Real rr_e = rates[k] - (cur[k] - ctl[k]) * hz;
        ctl[k] = cur[k];
        Real ir = clip_(ctl[6 + k] - rot_e[k] * dt, Real(-1500), Real(1500));
        if (k < 2) ir = clip_(ir, Real(-1), Real(1));
        ctl[6 + k] = ir;
        tq[k] = clip_(-K.p_tor[k] * rot_e[k] + K.d_tor[k] * rr_e + K.i_tor[k] * ir, Real(-3200), Real(3200));
    }
}

}  // namespace adrp
