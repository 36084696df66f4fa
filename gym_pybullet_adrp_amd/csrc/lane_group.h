// lane_group.h — the cross-lane and lane-mapping vocabulary of the kernels that run the N drones of an
// env on adjacent lanes (multihover_kernel.h, ctrl_kernel.h, race_kernel.h, race_quad.h), gfx950.
//
// Lane mapping: the N drones of env e are lanes [e G, e G + N) of the grid, G = the next power of two
// >= N, so a group is aligned and never straddles a wave (64 / G envs per wave).  Lanes n >= N of a
// group and groups past E are inactive: they run the same instruction stream on a benign state (the
// cross-lane moves need every lane of the wave in step), load nothing, store nothing, and every
// exchange or reduction masks them out by k < N.
#pragma once

#include "adrp_device.h"

namespace adrp {

template <typename Real>
struct Body;    // hover_dynamics.h
template <typename Real>
struct Chain;

constexpr int mh_group(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : 8; }

// value of lane k of this lane's group of G adjacent lanes (the drones of one env).  G <= 4: a
// DPP quad_perm move (one VALU op, no LDS round trip); G = 8: ds_bpermute.  k must fold to a
// constant (unrolled loops).
template <int G>
__device__ __forceinline__ int grp_bcast_i(int v, int k) {
    if constexpr (G == 1) {
        return v;
    } else if constexpr (G == 2) {
        switch (k) {   // quad_perm [k, k, 2 + k, 2 + k]
            case 0: return __builtin_amdgcn_mov_dpp(v, 0 | (0 << 2) | (2 << 4) | (2 << 6), 0xf, 0xf, false);
            default: return __builtin_amdgcn_mov_dpp(v, 1 | (1 << 2) | (3 << 4) | (3 << 6), 0xf, 0xf, false);
        }
    } else if constexpr (G == 4) {
        switch (k) {   // quad_perm [k, k, k, k]
            case 0: return __builtin_amdgcn_mov_dpp(v, 0x00, 0xf, 0xf, false);
            case 1: return __builtin_amdgcn_mov_dpp(v, 0x55, 0xf, 0xf, false);
            case 2: return __builtin_amdgcn_mov_dpp(v, 0xaa, 0xf, 0xf, false);
            default: return __builtin_amdgcn_mov_dpp(v, 0xff, 0xf, 0xf, false);
        }
    } else {
        return __shfl(v, k, G);
    }
}
template <int G>
__device__ __forceinline__ float grp_bcast(float v, int k) {
    return __int_as_float(grp_bcast_i<G>(__float_as_int(v), k));
}
template <int G>
__device__ __forceinline__ double grp_bcast(double v, int k) {
    const int lo = grp_bcast_i<G>(__double2loint(v), k), hi = grp_bcast_i<G>(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

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

// the downwash exponential: fp32 v_exp_f32; fp64 the table form (x <= 0)
__device__ __forceinline__ float dw_exp(float x, const double*) { return fexp_(x); }
__device__ __forceinline__ double dw_exp(double x, const double* tab) { return f64::exp_tab(x, tab); }

// _downwash (BaseAviary.py:792-818) as pyb_chain's external force, every sub-step from the group's
// current positions (:350-351 refreshes self.pos per sub-step in these modes).  Lane n takes its
// partners in the order n + 1, n + 2, ... (mod G): G - 1 terms, none for itself, and an order that
// depends on the drone's place in its env alone, not on E or on the env's place in the batch.  A term is
// alpha exp(-(dxy / beta)^2 / 2) with alpha = DW1 (PROP_RADIUS / (4 dz))^2, beta = DW2 dz + DW3;
// only dxy^2 enters, so no square root.  The force acts on link 4 along the z axis of the cached
// link basis (the current one, GND, once _groundEffect's getLinkStates has refreshed it), through the
// centre of mass: no torque.  N = 1 (G = 1) has no partner and no exchange.
template <typename Real, int G, bool GND>
struct Downwash {
    Real dw1, dw2, dw3, prop_r;   // DW_COEFF_1..3, PROP_RADIUS
    int n, N;
    __device__ __forceinline__ V3<Real> operator()(const Body<Real>& bb, const Chain<Real>& st) const {
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
    }
};

}  // namespace adrp
