// multihover_kernel.h — fused MultiHoverAviary env.step for gfx950: one lane per (env, drone), all
// PYB_FREQ/CTRL_FREQ sub-steps in registers with the downwash exchanged across the lanes of an env
// every sub-step, then per-drone obs rows, the env's reward / terminated / truncated and the per-env
// auto-reset, in ONE launch.
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   BaseAviary.step, _physics / _groundEffect / _drag / _downwash      envs/BaseAviary.py:262-387, 683-818
//   _preprocessAction (RPM, ONE_D_RPM), _computeObs                    envs/BaseRLAviary.py:160-239, 284-319
//   TARGET_POS, _computeReward / _computeTerminated / _computeTruncated  envs/MultiHoverAviary.py:71-130
//
// Lane mapping and inactive lanes: lane_group.h's header comment; the group moves and the downwash are
// its functions (shared with ctrl_kernel.h).  A live lane only ever reads lanes of its own group, so an
// env's results do not depend on E or on where the env sits in the batch.
//
// The sub-step body is hover_dynamics.h's (pyb_chain / pyb_substep / dyn_substep); the downwash enters it
// as one more world-frame force (pyb_substep's Fext).  State, ints and ring use HoverAviary's layout
// with E N columns, column e N + n; the per-env ints are replicated on the env's columns.
#pragma once

#include "hover_dynamics.h"
#include "lane_group.h"

namespace adrp {

// per-drone constants of a MultiHoverAviary handle (device-resident, behind HoverConst / HoverReset)
template <typename Real>
struct MultiConst {
    int N;
    Real dw1, dw2, dw3, prop_r;                 // DW_COEFF_1..3, PROP_RADIUS
    Real init_xyz[ADRP_MAX_DRONES][3], init_rpy[ADRP_MAX_DRONES][3];
    Real target[ADRP_MAX_DRONES][3];            // INIT_XYZS[n] + (0, 0, 1 / (n + 1))
};

// the column view of the [..][E N] state for load_body / store_body
template <typename Real>
__device__ __forceinline__ HoverArgs<Real> mh_columns(const HoverArgs<Real>& a, size_t EN) {
    HoverArgs<Real> ac = a;
    ac.E = int(EN);
    return ac;
}

// BaseAviary.reset of drone n of env e: HoverAviary's draw on the drone's own Philox stream
// (env_offset + e, drone, episode), about the drone's own initial pose
template <typename Real>
__device__ __forceinline__ void mh_reset_state(const HoverArgs<Real>& a, const HoverConst<Real>& C,
                                               const MultiConst<Real>& M, int e, int n, Body<Real>& b, int32_t& sc,
                                               int32_t& ep) {
    HoverReset<Real> r = *a.r;   // the noise widths; the pose is the drone's
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.init_xyz[k] = M.init_xyz[n][k];
        r.init_rpy[k] = M.init_rpy[n][k];
    }
    hover_reset_draw(r, a.seed, uint64_t(a.env_offset + e), TAG_HOVER_RESET | uint32_t(n), C, b, sc, ep);
}

// obs row of a drone whose action history is empty (after a reset: the ring is cleared)
__device__ __forceinline__ void mh_write_row_cleared(float* __restrict__ row, const float o12[12], int D) {
#pragma unroll
    for (int k = 0; k < 12; ++k) row[k] = o12[k];
    for (int k = 12; k < D; ++k) row[k] = 0.0f;
}
template <int A>
__device__ __forceinline__ void mh_clear_ring(float* __restrict__ ring, int B, size_t EN, size_t col) {
    for (int p = 0; p < B; ++p)
#pragma unroll
        for (int j = 0; j < A; ++j) ring[(size_t(p) * EN + col) * A + j] = 0.0f;
}

// a.E: envs; a.f / a.ist / a.ring: [..][E N] columns; a.act / a.obs / a.tobs: [E][N][.]; a.rew / a.term /
// a.trunc: [E].  Launch with kStepBlock (one wave) threads per workgroup, ceil(E G / 64) workgroups.
// B > 0: the ring length as a template parameter, so the ring is loaded at entry (off the sub-step
// chain's tail) and lives in registers, as in hover_step; B == 0: runtime ring length a.B, the ring part of
// the obs row copied from HBM after the sub-steps.
template <typename Real, int PH, int A, int G, int B>
__global__ void __launch_bounds__(kStepBlock) multihover_step_kernel(HoverArgs<Real> a, const MultiConst<Real>* mp) {
    static_assert(G == 1 || G == 2 || G == 4 || G == 8, "lane-group width");
    static_assert(kStepBlock == 64, "a workgroup is one wave: no group straddles it");
    constexpr bool DRAG = (PH == ADRP_PHYS_PYB_DRAG || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    constexpr bool DYN = (PH == ADRP_PHYS_DYN);
    constexpr bool GND = (PH == ADRP_PHYS_PYB_GND || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    constexpr bool DW = (PH == ADRP_PHYS_PYB_DW || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    const HoverConst<Real>& C = *a.c;
    const MultiConst<Real>& M = *mp;
    constexpr int BR = B > 0 ? B : 1;
    const int N = M.N, BB = B > 0 ? B : a.B, D = B > 0 ? 12 + B * A : a.D;
    // (spelled out in both grouped step kernels: behind a shared lane descriptor they measured 0.04-0.12 us slower)
    const int E = a.E;
    const long long t = (long long)blockIdx.x * kStepBlock + threadIdx.x;
    const long long eg = t / G;
    const int n = int(t % G);
    const bool live = eg < E && n < N;
    const int e = live ? int(eg) : 0;
    const size_t EN = size_t(E) * N, col = size_t(e) * N + n;   // (col is only used by live lanes)
    const HoverArgs<Real> ac = mh_columns(a, EN);
    // ---- loads (live lanes); inactive lanes hover at rest one metre up ----
    float act[A];
#pragma unroll
    for (int j = 0; j < A; ++j) act[j] = 0.0f;
    float ring[BR][A];
#pragma unroll
    for (int p = 0; p < BR; ++p)
#pragma unroll
        for (int j = 0; j < A; ++j) ring[p][j] = 0.0f;
    int32_t sc = 0, ep = 0, head = 0;
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
        if constexpr (A == 4) {
            const float4 v = reinterpret_cast<const float4*>(a.act)[col];
            act[0] = v.x; act[1] = v.y; act[2] = v.z; act[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < A; ++j) act[j] = a.act[col * A + j];
        }
#pragma unroll
        for (int p = 0; p < B; ++p) {   // (no-op for B == 0)
            if constexpr (A == 4) {
                const float4 v = reinterpret_cast<const float4*>(a.ring)[size_t(p) * EN + col];
                ring[p][0] = v.x; ring[p][1] = v.y; ring[p][2] = v.z; ring[p][3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < A; ++j) ring[p][j] = a.ring[(size_t(p) * EN + col) * A + j];
            }
        }
        sc = a.ist[HI_STEP * EN + col];
        ep = a.ist[HI_EPISODE * EN + col];
        head = a.ist[HI_RING_HEAD * EN + col];
        load_body(ac, int(col), b, lag, DRAG, DYN);
    }
    // the env's ints are drone 0's
    sc = grp_bcast_i<G>(sc, 0);
    ep = grp_bcast_i<G>(ep, 0);
    head = grp_bcast_i<G>(head, 0);
    // ---- _preprocessAction: RPM = HOVER_RPM * (1 + 0.05 a), the gain in float32 (NEP 50) ----
    Real rpm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rpm[i] = C.hover_rpm * Real(rpm_gain(act[A == 1 ? 0 : i]));
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
    if (touched && live && a.contact_count) atomicAdd(a.contact_count, 1);
    // ---- action ring: append this action at `head` (deque.append, BaseRLAviary.py:187) ----
    if (live) {
#pragma unroll
        for (int j = 0; j < A; ++j) a.ring[(size_t(head) * EN + col) * A + j] = act[j];
    }
    const int head1 = head + 1 == BB ? 0 : head + 1;
#pragma unroll
    for (int p = 0; p < B; ++p) {
        const bool hit = p == head;
#pragma unroll
        for (int j = 0; j < A; ++j) ring[p][j] = hit ? act[j] : ring[p][j];
    }
    // ---- obs / reward / terminated / truncated (MultiHoverAviary.py:75-130) ----
    float o12[12];
    const V3<Real> rpy = hover_obs12(C, b, o12);
    const Real dx = M.target[n][0] - b.pos.x, dy = M.target[n][1] - b.pos.y, dz = M.target[n][2] - b.pos.z;
    const Real d2 = dx * dx + dy * dy + dz * dz;
    const Real r1 = Real(2) - d2 * d2;
    const Real rew_n = r1 > Real(0) ? r1 : Real(0);
    const Real dist_n = sqrt_(d2);
    const int out_n = fabs_(b.pos.x) > Real(2.0) || fabs_(b.pos.y) > Real(2.0) || b.pos.z > Real(2.0) ||
                      fabs_(rpy.x) > Real(0.4) || fabs_(rpy.y) > Real(0.4);
    // the env's sums over its drones in ascending n, in registers, the same on every lane of the group
    Real rew = Real(0), dist = Real(0);
    int out = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const Real rk = grp_bcast<G>(rew_n, k), dk = grp_bcast<G>(dist_n, k);
        const int ok = grp_bcast_i<G>(out_n, k);
        if (k < N) {
            rew += rk;
            dist += dk;
            out |= ok;
        }
    }
    const bool te = dist < Real(1e-4);
    const bool tr = out != 0 || sc >= C.trunc_steps;
    if (live && n == 0) {
        a.rew[e] = float(rew);
        a.term[e] = te;
        a.trunc[e] = tr;
    }
    sc += C.S;
    const bool done = a.autoreset && (te || tr);
    if (!live) return;   // (no cross-lane move below)
    float* row = a.obs + col * size_t(D);
    if (done) {
        // the whole env resets in this launch: every drone's terminal row, a cleared ring, a new draw
        if (a.tobs) {
            if constexpr (B > 0) write_row<A, B>(a.tobs + col * size_t(D), o12, ring, head1);
            else write_row_generic<A>(a.tobs + col * size_t(D), o12, a.ring, BB, int(EN), int(col), head1, act, true);
        }
        mh_reset_state(a, C, M, e, n, b, sc, ep);
        hover_obs12(C, b, o12);
        mh_clear_ring<A>(a.ring, BB, EN, col);
        mh_write_row_cleared(row, o12, D);
    } else {
        if constexpr (B > 0) write_row<A, B>(row, o12, ring, head1);
        else write_row_generic<A>(row, o12, a.ring, BB, int(EN), int(col), head1, act, true);
    }
    store_body(ac, int(col), b, lag, DRAG, DYN);
    a.ist[HI_STEP * EN + col] = sc;
    a.ist[HI_EPISODE * EN + col] = ep;
    a.ist[HI_RING_HEAD * EN + col] = head1;
}

// What the reset kernels of the [..][E N] column layouts share (BaseAviary.reset -> _housekeeping ->
// _computeObs), one lane per column: the drone's new state drawn and stored, the env's step counter and
// episode, and the first twelve obs values.  False for a lane past the last column or of an env the mask
// leaves alone.  rpm_always: last_rpm_* is stored in every physics mode (the state-row envs), not only
// with drag.
template <typename Real>
__device__ __forceinline__ bool mh_reset_column(const HoverArgs<Real>& a, const MultiConst<Real>& M, bool rpm_always,
                                                size_t& EN, size_t& col, Body<Real>& b, float o12[12]) {
    EN = size_t(a.E) * M.N;
    col = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= EN) return false;
    const int e = int(col / M.N), n = int(col % M.N);
    if (a.mask && !a.mask[e]) return false;
    const HoverConst<Real>& C = *a.c;
    const bool dyn = C.physics == ADRP_PHYS_DYN;
    const bool drag = rpm_always || C.physics == ADRP_PHYS_PYB_DRAG || C.physics == ADRP_PHYS_PYB_GND_DRAG_DW;
    int32_t sc = 0, ep = a.ist[HI_EPISODE * EN + col];   // (replicated on the env's columns: the lane's own copy)
    mh_reset_state(a, C, M, e, n, b, sc, ep);
    store_body(mh_columns(a, EN), int(col), b, C.link_lag && !dyn, drag, dyn);
    a.ist[HI_STEP * EN + col] = sc;
    a.ist[HI_EPISODE * EN + col] = ep;
    hover_obs12(C, b, o12);
    return true;
}

// reset kernel, one lane per column; the ring of a reset env is cleared
template <typename Real, int A>
__global__ void __launch_bounds__(256) multihover_reset_kernel(HoverArgs<Real> a, const MultiConst<Real>* mp) {
    size_t EN, col;
    Body<Real> b;
    float o12[12];
    if (!mh_reset_column(a, *mp, false, EN, col, b, o12)) return;
    mh_clear_ring<A>(a.ring, a.B, EN, col);
    mh_write_row_cleared(a.obs + col * size_t(a.D), o12, a.D);
}

}  // namespace adrp
