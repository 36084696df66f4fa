// plan_kernel.h — the scripted racer's spline planner on the device (include/adrp.h adrp_race_plan;
// gym_pybullet_adrp_amd/hardcoded.py planner="device"), included by plan.hip alone.
//
// Replaces, for the GPU batch, the host loop of HardCodedCommander.replan: one scipy splprep / splev per
// (env, drone) of a wave.  One launch per wave, two phases per workgroup of one wave (64 lanes):
//   fit:     one lane per (env, drone) slot runs spline_plan.h's fit on its own observation row.  The working set
//            (about 470 doubles, indexed at run time) lives in scratch: at 64 lanes it would not fit the CU's LDS,
//            and the kernel runs once per wave of races, not per step.  The result (n, t[20], c[3][16]) is parked
//            in LDS.
//   samples: the 64 lanes together write each planned slot's [L][3] samples: lane j evaluates parameters j, j + 64,
//            ... from the parked knots and coefficients (an LDS broadcast read) and stores three consecutive
//            doubles, so a wave's stores cover one contiguous 1,536-byte run of ref.
// Plain loads, selects and vector stores: no atomics.  Lanes past E * N, and the lanes of unmasked envs, compute
// nothing and store nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/adrp.h"
#include "spline_plan.h"

namespace adrp {

constexpr int kPlanLanes = 64;
constexpr int kPlanPoints = adrp_plan::kHardPoints;                       // 16 waypoints
constexpr int kPlanKnots = kPlanPoints + adrp_plan::kK1;                  // ADRP_PLAN_KNOTS
constexpr int kPlanCoef = kPlanPoints;                                    // ADRP_PLAN_COEF
static_assert(kPlanKnots == ADRP_PLAN_KNOTS && kPlanCoef == ADRP_PLAN_COEF, "include/adrp.h and spline_plan.h disagree");

__global__ void __launch_bounds__(kPlanLanes) race_plan_kernel(adrp_race_plan_io io) {
    __shared__ double sh_t[kPlanLanes][kPlanKnots];
    __shared__ double sh_c[kPlanLanes][3 * kPlanCoef];
    __shared__ int sh_n[kPlanLanes];          // 0: the slot is not planned
    const int E = io.num_envs, N = io.num_drones, L = io.ref_len;
    const long long EN = (long long)E * N;
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kPlanLanes;
    const long long slot = base + tid;
    bool active = slot < EN;
    if (active && io.mask) active = io.mask[slot / N] != 0;
    int flags = 0, n = 0, iters = 0;
    if (active) {
        adrp_plan::Work<kPlanPoints> work;
        adrp_plan::Spline<kPlanPoints> sp;
        adrp_plan::hardcoded_fit(io.obs + size_t(slot) * size_t(io.obs_stride), work, sp);
        flags = sp.flags;
        n = sp.n;
        iters = sp.iters;
        for (int i = 0; i < kPlanKnots; ++i) sh_t[tid][i] = sp.t[i];
        for (int d = 0; d < 3; ++d)
            for (int i = 0; i < kPlanCoef; ++i) sh_c[tid][d * kPlanCoef + i] = sp.c[d][i];
        if (io.knots)
            for (int i = 0; i < kPlanKnots; ++i) io.knots[size_t(slot) * kPlanKnots + i] = sp.t[i];
        if (io.n_knots) io.n_knots[slot] = n;
        if (io.coef)
            for (int i = 0; i < 3 * kPlanCoef; ++i) io.coef[size_t(slot) * 3 * kPlanCoef + i] = sp.c[i / kPlanCoef][i % kPlanCoef];
        if (io.phase) {
            io.phase[slot] = 0;
            io.phase[EN + slot] = 0;
            io.phase[2 * EN + slot] = 0;
        }
    }
    sh_n[tid] = n;
    __syncthreads();
    for (int d = 0; d < kPlanLanes; ++d) {
        const int nd = sh_n[d];               // uniform over the wave
        if (nd == 0) continue;
        double* __restrict__ out = io.ref + size_t(base + d) * size_t(L) * 3;
        bool high = false;
        for (int j = tid; j < L; j += kPlanLanes) {
            double p[3];
            adrp_plan::spline_eval(sh_t[d], sh_c[d], kPlanCoef, nd, io.samples[j], p);
            out[size_t(j) * 3 + 0] = p[0];
            out[size_t(j) * 3 + 1] = p[1];
            out[size_t(j) * 3 + 2] = p[2];
            high = high || !(p[2] < adrp_plan::kCeiling);
        }
        const bool any_high = __any(high ? 1 : 0) != 0;
        if (tid == d && any_high) flags |= adrp_plan::kStatCeiling;
    }
    if (active) io.status[slot] = adrp_plan::status_word(flags, n, iters);
}

}  // namespace adrp
