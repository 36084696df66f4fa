// ctrl_kernel.h — fused CtrlAviary / VelocityAviary env.step for gfx950: one lane per (env, drone), all
// PYB_FREQ/CTRL_FREQ sub-steps in registers with the downwash exchanged across the lanes of an env every
// sub-step, then the 20-float drone state row (_getDroneStateVector) per drone, in ONE launch.
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   BaseAviary.step, _getDroneStateVector                    envs/BaseAviary.py:262-387, 553-573
//   CtrlAviary._preprocessAction (clip to [0, MAX_RPM])      envs/CtrlAviary.py:121-140
//   VelocityAviary._preprocessAction (DSLPIDControl)         envs/VelocityAviary.py:129-168
//   reward -1, terminated / truncated False                  envs/CtrlAviary.py:144-185
//
// Lane mapping and inactive lanes are multihover_step_kernel's (lane_group.h): groups of G aligned lanes
// (G = the next power of two >= N), a workgroup is one wave, lanes n >= N and groups past E run the same
// instruction stream on a benign state (at rest one metre up, zero action: zero RPMs, or for
// VelocityAviary the zero-direction target velocity), load nothing and store nothing.  The downwash
// exchange is the one Downwash functor of lane_group.h that multihover_step_kernel calls too.
//
// State: HoverAviary's base float fields with E N columns, column e N + n, no action ring (these envs
// have no action history); last_rpm_* is written in every physics mode (it is the obs row's last four
// columns); VelocityAviary adds the nine pid_* fields, one DSLPIDControl per drone, which a reset keeps
// (the reference builds the controllers once, VelocityAviary.py:62).  The episode never ends: reward
// -1, both flags 0, no auto-reset.
#pragma once

#include "multihover_kernel.h"

namespace adrp {

// per-drone constants of a CtrlAviary / VelocityAviary handle (device-resident, behind HoverConst /
// HoverReset): MultiHoverAviary's block (its targets unused) and the RPM clip
template <typename Real>
struct CtrlConst {
    MultiConst<Real> m;
    Real max_rpm;   // MAX_RPM = sqrt(THRUST2WEIGHT g m / (4 KF)) (BaseAviary.py:120)
};

constexpr int kCtrlObs = 20;   // pos 3, quat 4 (xyzw), rpy 3, vel 3, ang_v 3, last_clipped_action 4

// the 80-byte row of one drone (16-byte aligned: col * 80), five 16-byte stores from registers
template <typename Real>
__device__ __forceinline__ void ctrl_write_row(float* __restrict__ row, const float o12[12], const Q4<Real>& q,
                                               const Real rpm[4]) {
    float4* r4 = reinterpret_cast<float4*>(row);
    r4[0] = make_float4(o12[0], o12[1], o12[2], float(q.x));
    r4[1] = make_float4(float(q.y), float(q.z), float(q.w), o12[3]);
    r4[2] = make_float4(o12[4], o12[5], o12[6], o12[7]);
    r4[3] = make_float4(o12[8], o12[9], o12[10], o12[11]);
    r4[4] = make_float4(float(rpm[0]), float(rpm[1]), float(rpm[2]), float(rpm[3]));
}

// CTL = 0 (CtrlAviary): the action is the four motor speeds, a.act float32 [E][N][4], or, when rpm_real
// is not null, [E][N][4] in the handle's own precision (adrp_step_rpm: a float64 handle takes float64
// RPMs unrounded).  CTL = ADRP_ACT_VEL (VelocityAviary): a.act float32 [E][N][4] velocity commands.
// a.f / a.ist: [..][E N] columns; a.obs: [E][N][20]; a.rew / a.term / a.trunc: [E].  Launch with
// kStepBlock (one wave) threads per workgroup, ceil(E G / 64) workgroups.
template <typename Real, int PH, int G, int CTL>
__global__ void __launch_bounds__(kStepBlock) ctrl_step_kernel(HoverArgs<Real> a, const CtrlConst<Real>* kp,
                                                               const Real* __restrict__ rpm_real) {
    static_assert(CTL == 0 || CTL == ADRP_ACT_VEL, "raw RPMs or the fused velocity controller");
    static_assert(G == 1 || G == 2 || G == 4 || G == 8, "lane-group width");
    static_assert(kStepBlock == 64, "a workgroup is one wave: no group straddles it");
    constexpr bool DRAG = (PH == ADRP_PHYS_PYB_DRAG || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    constexpr bool DYN = (PH == ADRP_PHYS_DYN);
    constexpr bool GND = (PH == ADRP_PHYS_PYB_GND || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    constexpr bool DW = (PH == ADRP_PHYS_PYB_DW || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    const HoverConst<Real>& C = *a.c;
    const MultiConst<Real>& M = kp->m;
    const int N = M.N;
    // (spelled out in both grouped step kernels: behind a shared lane descriptor they measured 0.04-0.12 us slower)
    const int E = a.E;
    const long long t = (long long)blockIdx.x * kStepBlock + threadIdx.x;
    const long long eg = t / G;
    const int n = int(t % G);
    const bool live = eg < E && n < N;
    const int e = live ? int(eg) : 0;
    const size_t EN = size_t(E) * N, col = size_t(e) * N + n;   // (col is only used by live lanes)
    const HoverArgs<Real> ac = mh_columns(a, EN);
    // ---- loads (live lanes); inactive lanes rest one metre up with a zero action ----
    float act[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    Real rpm[4] = {Real(0), Real(0), Real(0), Real(0)};
    Real ctl[HF_NPID];
#pragma unroll
    for (int k = 0; k < HF_NPID; ++k) ctl[k] = Real(0);
    int32_t sc = 0;
    const bool lag = C.link_lag && !DYN;
    Body<Real> b;   // (spelled out too: behind a function call the float64 PYB_DRAG G = 8 kernel takes two more AGPRs)
    b.pos = v3(Real(0), Real(0), Real(1));
    b.q = {Real(0), Real(0), Real(0), Real(1)};
    b.ql = b.q;
    b.vel = v3(Real(0), Real(0), Real(0));
    b.w = b.vel;
    b.angv = b.vel;
#pragma unroll
    for (int i = 0; i < 4; ++i) b.prev_rpm[i] = Real(0);
    if (live) {
        if (CTL == 0 && rpm_real) {
#pragma unroll
            for (int i = 0; i < 4; ++i) rpm[i] = rpm_real[col * 4 + i];
        } else {
            const float4 v = reinterpret_cast<const float4*>(a.act)[col];
            act[0] = v.x; act[1] = v.y; act[2] = v.z; act[3] = v.w;
#pragma unroll
            for (int i = 0; i < 4; ++i) rpm[i] = Real(act[i]);
        }
        sc = a.ist[HI_STEP * EN + col];
        load_body(ac, int(col), b, lag, DRAG, DYN);
        if constexpr (CTL != 0) {
#pragma unroll
            for (int k = 0; k < HF_NPID; ++k) ctl[k] = a.f[(HF_PID + k) * EN + col];
        }
    }
    // ---- _preprocessAction ----
    if constexpr (CTL != 0) {
        dslpid_rpm<Real, CTL>(C, b, act, ctl, rpm);   // on the state at the start of the step
    } else {
        const Real hi = kp->max_rpm;                   // np.clip(action, 0, MAX_RPM)
#pragma unroll
        for (int i = 0; i < 4; ++i) rpm[i] = rpm[i] < Real(0) ? Real(0) : (rpm[i] > hi ? hi : rpm[i]);
    }
    // ---- sub-step loop (BaseAviary.py:347-376) ----
    bool touched = false;
    if constexpr (DYN) {
        for (int s = 0; s < C.S; ++s) dyn_substep(C, b, rpm);
    } else if constexpr (DW) {
        const Downwash<Real, G, GND> downwash = {M.dw1, M.dw2, M.dw3, M.prop_r, n, N};
        touched = pyb_chain<Real, PH, 0, DRAG>(C, b, rpm, lag, downwash);
    } else {
        touched = pyb_chain<Real, PH, 0, DRAG>(C, b, rpm, lag, NoExtForce{});
    }
    if (!live) return;   // (no cross-lane move below)
    if (touched && a.contact_count) atomicAdd(a.contact_count, 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) b.prev_rpm[i] = rpm[i];   // last_clipped_action, in every physics mode
    // ---- the state row; reward -1, never terminated or truncated ----
    float o12[12];
    hover_obs12(C, b, o12);
    ctrl_write_row(a.obs + col * size_t(kCtrlObs), o12, b.q, rpm);
    if (n == 0) {
        a.rew[e] = -1.0f;
        a.term[e] = 0;
        a.trunc[e] = 0;
    }
    store_body(ac, int(col), b, lag, true, DYN);
    if constexpr (CTL != 0) {
#pragma unroll
        for (int k = 0; k < HF_NPID; ++k) a.f[(HF_PID + k) * EN + col] = ctl[k];
    }
    a.ist[HI_STEP * EN + col] = sc + C.S;
}

// reset kernel (BaseAviary.reset -> _housekeeping -> _computeObs), one lane per column: the drone's
// initial pose (+ the init_*_noise extension on its own Philox stream), zero RPM columns; the pid_*
// fields are left as they are
template <typename Real>
__global__ void __launch_bounds__(256) ctrl_reset_kernel(HoverArgs<Real> a, const CtrlConst<Real>* kp) {
    size_t EN, col;
    Body<Real> b;
    float o12[12];
    if (!mh_reset_column(a, kp->m, true, EN, col, b, o12)) return;
    ctrl_write_row(a.obs + col * size_t(kCtrlObs), o12, b.q, b.prev_rpm);
}

}  // namespace adrp
