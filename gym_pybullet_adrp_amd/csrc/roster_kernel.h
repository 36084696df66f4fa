// roster_kernel.h — device kernels of the race rosters (include/adrp.h: adrp_race_roster_*;
// gym_pybullet_adrp_amd/rollout.py RosterRolloutCollector), included by roster.hip alone.
//
// A roster gives every drone of a MultiRaceAviary one role: a sample of the policy being trained, the scripted
// HardCodedController, a frozen policy, or none.  A collector resets its envs one by one, so the scripted drones'
// take-off, spline index, notify and land phases follow their own env's clock (sim_kernel.h's controller kernel
// takes one episode time for a whole wave), and only the learner drones' columns are kept (agents_kernel.h's step
// writes all E N).  The per-slot bodies are race_slot.h's, shared with those two kernels.
// One lane per slot; plain loads, selects and vector stores; lanes past the end return before any load.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/adrp.h"
#include "race_slot.h"

namespace adrp {

constexpr int kRosterLanes = 256;

// learner l is drone drone[l] (the inverse of adrp_race_roster_io.learner_index, made by the host)
struct RosterLearners {
    int32_t drone[ADRP_MAX_DRONES];
};

// adrp_race_roster_act: one lane per (env, drone) slot e * N + n.  The clock is only read here.
__global__ void __launch_bounds__(kRosterLanes) race_roster_act_kernel(adrp_race_roster_io io) {
    const int E = io.num_envs, N = io.num_drones, EN = E * N;
    const int slot = blockIdx.x * kRosterLanes + threadIdx.x;
    if (slot >= EN) return;
    const int e = slot / N, n = slot - e * N;
    const double ep_time = double(io.clock[e]) / io.ctrl_freq;
    const int role = io.role[n];
    // LEARNER is POLICY's transform of the learner's own env action
    const bool learner = role == ADRP_ROSTER_LEARNER;
    const int kind = learner ? ADRP_RACE_CTRL_POLICY : role;
    const float4* sp = nullptr;
    if (learner) sp = reinterpret_cast<const float4*>(io.learner_act) + (size_t(io.learner_index[n]) * E + e);
    else if (role == ADRP_ROSTER_POLICY) sp = reinterpret_cast<const float4*>(io.setpoints) + (size_t(n) * E + e);
    race_controller_slot(slot, EN, kind, sp, io.ref_len, io.ref, io.offset, io.phase, ep_time, io.codes, io.args);
}

// adrp_race_roster_tick: one lane per slot; the n == 0 lane owns its env's clock
__global__ void __launch_bounds__(kRosterLanes) race_roster_tick_kernel(adrp_race_roster_io io, const uint8_t* __restrict__ mask) {
    const int E = io.num_envs, N = io.num_drones, EN = E * N;
    const int slot = blockIdx.x * kRosterLanes + threadIdx.x;
    if (slot >= EN) return;
    const int e = slot / N, n = slot - e * N;
    const bool reset = !mask || mask[e] != 0;
    if (reset) {
        io.phase[slot] = 0;
        io.phase[EN + slot] = 0;
        io.phase[2 * EN + slot] = 0;
    }
    if (n == 0) io.clock[e] = reset ? 0 : io.clock[e] + 1;
}

// adrp_race_roster_step: one lane per learner column c = l * E + e, on the state of slot e * N + drone[l]
__global__ void __launch_bounds__(kRosterLanes) race_roster_step_kernel(
    adrp_race_agents_io io, RosterLearners who, int num_learners, const float* __restrict__ obs, const int32_t* __restrict__ gate,
    const int32_t* __restrict__ flags, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
    const float* __restrict__ boot_value, double gamma, float* __restrict__ rewards, uint8_t* __restrict__ valid,
    float* __restrict__ next_start, double* __restrict__ ep_return, int32_t* __restrict__ ep_length) {
    const int E = io.num_envs;
    const int c = blockIdx.x * kRosterLanes + threadIdx.x;
    if (c >= num_learners * E) return;
    const int l = c / E, e = c - l * E;
    const int j = e * io.num_drones + who.drone[l];
    race_agent_step_slot(io, j, e, c, obs, gate, flags, term, trunc, boot_value, gamma, rewards, valid, next_start, ep_return,
                         ep_length);
}

// adrp_race_roster_done: one lane per env, after the step kernel above has updated alive.  The env ends with its
// race (term | trunc) or with its last learner; only the learner slots' alive is read.
__global__ void __launch_bounds__(kRosterLanes) race_roster_done_kernel(
    int num_envs, int num_drones, RosterLearners who, int num_learners, const uint8_t* __restrict__ alive,
    const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc, uint8_t* __restrict__ mask_out) {
    const int e = blockIdx.x * kRosterLanes + threadIdx.x;
    if (e >= num_envs) return;
    bool any = false;
    for (int l = 0; l < num_learners; ++l) any = any || alive[size_t(e) * num_drones + who.drone[l]] != 0;
    mask_out[e] = ((term[e] | trunc[e]) != 0 || !any) ? 1 : 0;
}

}  // namespace adrp
