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
// Lane mapping: the N drones of env e are lanes [e G, e G + N) of the grid, G = the next power of
// two >= N, so a group is aligned and never straddles a wave (64 / G envs per wave).  Lanes n >= N of
// a group and groups past E are inactive: they run the same instruction stream on a benign state (the
// cross-lane moves below need every lane of the wave in step), load nothing, store nothing, and every
// exchange or reduction masks them out by k < N.  A live lane only ever reads lanes of its own group,
// so an env's results do not depend on E or on where the env sits in the batch.
//
// The sub-step body is hover_kernel.h's (pyb_chain / pyb_substep / dyn_substep); the downwash enters it
// as one more world-frame force (pyb_substep's Fext).  State, ints and ring use HoverAviary's layout
// with E N columns, column e N + n; the per-env ints are replicated on the env's columns.
#pragma once

#include "hover_kernel.h"
#include "race_kernel.h"   // grp_bcast: DPP quad_perm (G <= 4) / ds_bpermute (G = 8) group broadcast (the reductions)
#include "race_quad.h"     // dw_exp

namespace adrp {

// per-drone constants of a MultiHoverAviary handle (device-resident, behind HoverConst / HoverReset)
template <typename Real>
struct MultiConst {
    int N;
    Real dw1, dw2, dw3, prop_r;                 // DW_COEFF_1..3, PROP_RADIUS
    Real init_xyz[ADRP_MAX_DRONES][3], init_rpy[ADRP_MAX_DRONES][3];
    Real target[ADRP_MAX_DRONES][3];            // INIT_XYZS[n] + (0, 0, 1 / (n + 1))
};

constexpr int mh_group(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : 8; }

// value of lane (n + r) mod G of this lane's group of G adjacent lanes, n the lane's place in the group,
// 0 < r < G.  G <= 4: one DPP quad_perm move (a rotation of the quad, or of its halves); G = 8:
// ds_bpermute.  r must fold to a constant (unrolled loops).
template <int G>
__device__ __forceinline__ int grp_rot_i(int v, int r, int n) {
    if constexpr (G == 2) {
        return __builtin_amdgcn_mov_dpp(v, 0xb1, 0xf, 0xf, false);   // quad_perm [1, 0, 3, 2]
    } else if constexpr (G == 4) {
        switch (r) {
            case 1: return __builtin_amdgcn_mov_dpp(v, 0x39, 0xf, 0xf, false);    // [1, 2, 3, 0]
            case 2: return __builtin_amdgcn_mov_dpp(v, 0x4e, 0xf, 0xf, false);    // [2, 3, 0, 1]
            default: return __builtin_amdgcn_mov_dpp(v, 0x93, 0xf, 0xf, false);   // [3, 0, 1, 2]
        }
    } else {
        return __shfl(v, (n + r) & (G - 1), G);
    }
}
template <int G>
__device__ __forceinline__ float grp_rot(float v, int r, int n) {
    return __int_as_float(grp_rot_i<G>(__float_as_int(v), r, n));
}
template <int G>
__device__ __forceinline__ double grp_rot(double v, int r, int n) {   // a 64-bit value goes as two 32-bit moves
    const int lo = grp_rot_i<G>(__double2loint(v), r, n), hi = grp_rot_i<G>(__double2hiint(v), r, n);
    return __hiloint2double(hi, lo);
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
    const int N = M.N, E = a.E, BB = B > 0 ? B : a.B, D = B > 0 ? 12 + B * A : a.D;
    const long long t = (long long)blockIdx.x * kStepBlock + threadIdx.x;
    const long long eg = t / G;
    const int n = int(t % G);
    const bool live = eg < E && n < N;
    const int e = live ? int(eg) : 0;
    const size_t EN = size_t(E) * N, col = size_t(e) * N + n;   // (col is only used by live lanes)
    HoverArgs<Real> ac = a;   // the column view of the state for load_body / store_body
    ac.E = int(EN);
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
    Body<Real> b;
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
        // _downwash (BaseAviary.py:792-818), every sub-step from the group's current positions (:350-351
        // refreshes self.pos per sub-step in these modes).  Lane n takes its partners in the order n + 1,
        // n + 2, ... (mod G): G - 1 terms, none for itself, and an order that depends on the drone's place in
        // its env alone, not on E or on the env's place in the batch.  A term is
        // alpha exp(-(dxy / beta)^2 / 2) with alpha = DW1 (PROP_RADIUS / (4 dz))^2, beta = DW2 dz + DW3;
        // only dxy^2 enters, so no square root.  The force acts on link 4 along the z axis of the cached
        // link basis (the current one once _groundEffect's getLinkStates has refreshed it), through the
        // centre of mass: no torque.  N = 1 (G = 1) has no partner and no exchange.
        const Real dw1 = M.dw1, dw2 = M.dw2, dw3 = M.dw3, prop_r = M.prop_r;
        auto downwash = [&](const Body<Real>& bb, const Chain<Real>& st) {
            Real tsum = Real(0);
#pragma unroll
            for (int r = 1; r < G; ++r) {
                const int k = (n + r) & (G - 1);
                const Real ox = grp_rot<G>(bb.pos.x, r, n), oy = grp_rot<G>(bb.pos.y, r, n), oz = grp_rot<G>(bb.pos.z, r, n);
                const Real dz = oz - bb.pos.z, dx = ox - bb.pos.x, dy = oy - bb.pos.y;
                const Real dxy2 = dx * dx + dy * dy;
                const Real kk = prop_r * rcp_nc_(Real(4) * dz);
                const Real rb = rcp_nc_(dw2 * dz + dw3);
                const Real term = dw1 * kk * kk * dw_exp(Real(-0.5) * (dxy2 * rb * rb), f64::kExp2Tab32);
                tsum += (k < N && dz > Real(0) && dxy2 < Real(100)) ? term : Real(0);
            }
            const V3<Real> z = GND ? st.zc : st.zs;
            return v3(-tsum * z.x, -tsum * z.y, -tsum * z.z);
        };
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

// reset kernel (BaseAviary.reset -> _housekeeping -> _computeObs), one lane per column; the ring of a
// reset env is cleared
template <typename Real, int A>
__global__ void __launch_bounds__(256) multihover_reset_kernel(HoverArgs<Real> a, const MultiConst<Real>* mp) {
    const MultiConst<Real>& M = *mp;
    const size_t EN = size_t(a.E) * M.N;
    const size_t col = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= EN) return;
    const int e = int(col / M.N), n = int(col % M.N);
    if (a.mask && !a.mask[e]) return;
    const HoverConst<Real>& C = *a.c;
    const bool dyn = C.physics == ADRP_PHYS_DYN;
    const bool drag = C.physics == ADRP_PHYS_PYB_DRAG || C.physics == ADRP_PHYS_PYB_GND_DRAG_DW;
    HoverArgs<Real> ac = a;
    ac.E = int(EN);
    Body<Real> b;
    int32_t sc = 0, ep = a.ist[HI_EPISODE * EN + col];   // (replicated on the env's columns: the lane's own copy)
    mh_reset_state(a, C, M, e, n, b, sc, ep);
    store_body(ac, int(col), b, C.link_lag && !dyn, drag, dyn);
    a.ist[HI_STEP * EN + col] = sc;
    a.ist[HI_EPISODE * EN + col] = ep;
    float o12[12];
    hover_obs12(C, b, o12);
    mh_clear_ring<A>(a.ring, a.B, EN, col);
    mh_write_row_cleared(a.obs + col * size_t(a.D), o12, a.D);
}

}  // namespace adrp
