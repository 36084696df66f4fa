// sim_kernel.h — the two per-step kernels of the batched race evaluation (include/adrp.h adrp_race_controllers /
// adrp_race_results_*; gym_pybullet_adrp_amd/sim.py), included by sim.hip alone.
//
// Replaces, for the GPU batch, what scripts/sim.py:68-108 does on the host once per env.step:
//   * race_controller_kernel: `actions = [a.predict(obs[i], ep_time=sim_time) for i, a in enumerate(agents)]` (:93)
//     for the agents HardCodedController (user_controller/HardCodedController.py:117-190) and RLController
//     (RLController.py:39-73: `_action_transform`'s FULLSTATE tuple); the PPO actor itself ran before this launch
//     (adrp_policy_act into the setpoint buffer).
//   * race_results_kernel: `stats["episode_rewards"][run] += reward`, the `while not (terminated or truncated)`
//     test and `stats["episode_times"][run] = sim_time` (:78, 102, 108), plus the per-drone outcome (gates passed,
//     finish step, elimination step) that the reference leaves in env.current_gate / drones_eliminated.
// Both are plain loads, selects and vector stores: no atomics, no LDS traffic beyond one fixed-order count.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/adrp.h"
#include "race_slot.h"

namespace adrp {

constexpr int kCtrlLanes = 256;
constexpr int kResLanes = 1024, kResWaves = kResLanes / 64;

// One lane per (env, drone) slot e * N + n.  Every slot of codes / args is written on every step (race_slot.h:
// the body, shared with the roster collector's act kernel, which takes the episode time per env).
__global__ void __launch_bounds__(kCtrlLanes) race_controller_kernel(adrp_race_ctrl_io io, double ep_time) {
    const int E = io.num_envs, N = io.num_drones, EN = E * N;
    const int slot = blockIdx.x * kCtrlLanes + threadIdx.x;
    if (slot >= EN) return;
    const int e = slot / N, n = slot - e * N;
    const float4* sp = io.kind[n] == ADRP_RACE_CTRL_POLICY ? reinterpret_cast<const float4*>(io.setpoints) + (size_t(n) * E + e) : nullptr;
    race_controller_slot(slot, EN, io.kind[n], sp, io.ref_len, io.ref, io.offset, io.phase, ep_time, io.codes, io.args);
}

// Fixed-order count over one workgroup: wave shuffles, then the sixteen wave sums in index order.
__device__ __forceinline__ int block_count(int v, int* sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < kResWaves; ++w) r += sh[w];
    __syncthreads();   // sh is reused by the next count
    return r;
}

// adrp_race_results_begin: open a wave.  The running arrays go to zero, finish / elim to -1, env e is open
// when e < n_open.
__global__ void __launch_bounds__(kResLanes) race_results_begin_kernel(adrp_race_results_io io, int n_open) {
    const int E = io.num_envs, N = io.num_drones;
    for (int e = threadIdx.x; e < E; e += kResLanes) {
        io.run_return[e] = 0.0;
        io.run_length[e] = 0;
        io.open[e] = e < n_open ? 1 : 0;
        for (int n = 0; n < N; ++n) {
            io.gates[e * N + n] = 0;
            io.finish[e * N + n] = -1;
            io.elim[e * N + n] = -1;
        }
    }
    if (threadIdx.x == 0) io.meta[1] = n_open;
}

// One launch (one workgroup, strided over the envs) per env.step, after it.  gate / flags: the race state's
// per-drone ints, slot e * N + n (flags bit 0 eliminated, bit 1 finished).
__global__ void __launch_bounds__(kResLanes) race_results_kernel(adrp_race_results_io io, const int32_t* __restrict__ gate,
                                                                 const int32_t* __restrict__ flags,
                                                                 const float* __restrict__ rew,
                                                                 const uint8_t* __restrict__ term,
                                                                 const uint8_t* __restrict__ trunc) {
    __shared__ int sh[kResWaves];
    const int E = io.num_envs, N = io.num_drones;
    int still = 0, closed = 0;
    for (int e = threadIdx.x; e < E; e += kResLanes) {
        if (!io.open[e]) continue;
        const double ret = io.run_return[e] + double(rew[e]);
        const int len = io.run_length[e] + 1;
        io.run_return[e] = ret;
        io.run_length[e] = len;
        const bool te = term[e] != 0, tr = trunc[e] != 0, done = te || tr;
        const long long slot = (long long)io.base + e;
        const bool log = done && slot < io.capacity;   // (begin checked base + n_open <= capacity: always true then)
        for (int n = 0; n < N; ++n) {
            const int j = e * N + n;
            const int g = gate[j], f = flags[j];
            int fin = io.finish[j], el = io.elim[j];
            if ((f & 2) && fin < 0) fin = len;
            if ((f & 1) && el < 0) el = len;
            io.gates[j] = g;
            io.finish[j] = fin;
            io.elim[j] = el;
            if (log) {
                io.log_gates[slot * N + n] = g;
                io.log_finish[slot * N + n] = fin;
                io.log_elim[slot * N + n] = el;
            }
        }
        if (log) {
            io.log_return[slot] = ret;
            io.log_length[slot] = len;
            io.log_term[slot] = te ? 1 : 0;
            io.log_trunc[slot] = tr ? 1 : 0;
        }
        if (done) {
            io.open[e] = 0;
            closed += 1;
        } else {
            still += 1;
        }
    }
    still = block_count(still, sh);
    closed = block_count(closed, sh);
    if (threadIdx.x == 0) {
        io.meta[0] += closed;
        io.meta[1] = still;
        io.meta[2] += 1;
    }
}

}  // namespace adrp
