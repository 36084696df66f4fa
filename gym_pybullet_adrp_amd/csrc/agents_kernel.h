// agents_kernel.h — device kernels of the per-drone race agents (include/adrp.h: adrp_race_agents_*;
// gym_pybullet_adrp_amd/rollout.py MultiAgentRolloutCollector), included by agents.hip alone.
//
// What the reference cannot do (its README: one agent at a time in MultiRaceAviary) needs, per drone and per
// env.step: utils/wrapper.py:121-186 RewardWrapper._compute_reward on the drone's own row (the race step kernel
// fuses it for drone 0 alone, race_quad.h), the drone's own episode end (eliminated or finished while the env
// goes on), the validity of a dead drone's samples, SB3's time-limit bootstrap and the episode starts GAE reads.
// One lane per agent slot j = e * N + n; plain loads, selects and vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/adrp.h"

constexpr int kAgentLanes = 256;

// adrp_race_agents_reset: RewardWrapper.reset per drone of the masked envs
__global__ void __launch_bounds__(kAgentLanes) race_agents_reset_kernel(adrp_race_agents_io io, const float* __restrict__ obs,
                                                                        const uint8_t* __restrict__ mask) {
    const int j = blockIdx.x * kAgentLanes + threadIdx.x;
    if (j >= io.num_envs * io.num_drones) return;
    if (mask && mask[j / io.num_drones] == 0) return;
    const float* __restrict__ row = obs + size_t(j) * io.obs_dim;
    io.wr_gate[j] = int(row[48]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        io.wr_target[3 * j + k] = double(row[12 + k]);
        io.wr_prev[3 * j + k] = double(row[k]);
    }
    io.alive[j] = 1;
    io.run_return[j] = 0.0;
    io.run_length[j] = 0;
}

// adrp_race_agents_step: the reward's arithmetic is race_quad.h's drone-0 copy (oracle/race.c race_reward_wrapper)
// in float64 on the float32 row, with the drone's own "became done" / "finished" for terminated / task_completed
__global__ void __launch_bounds__(kAgentLanes) race_agents_step_kernel(
    adrp_race_agents_io io, const float* __restrict__ obs, const int32_t* __restrict__ gate, const int32_t* __restrict__ flags,
    const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc, const float* __restrict__ boot_value, double gamma,
    float* __restrict__ rewards, uint8_t* __restrict__ valid, float* __restrict__ next_start, double* __restrict__ ep_return,
    int32_t* __restrict__ ep_length) {
    const int j = blockIdx.x * kAgentLanes + threadIdx.x;
    if (j >= io.num_envs * io.num_drones) return;
    const int e = j / io.num_drones;
    const float* __restrict__ row = obs + size_t(j) * io.obs_dim;
    const bool was_alive = io.alive[j] != 0;
    const int fl = flags[j];
    const bool done_now = (fl & 3) != 0, fin = (fl & 2) != 0;
    const bool newly = was_alive && done_now;
    const bool te = term[e] != 0, tr = trunc[e] != 0;

    const int gate_id = gate[j];
    int wr_gate = io.wr_gate[j];
    double tgt[3] = {io.wr_target[3 * j], io.wr_target[3 * j + 1], io.wr_target[3 * j + 2]};
    const double prv[3] = {io.wr_prev[3 * j], io.wr_prev[3 * j + 1], io.wr_prev[3 * j + 2]};
    const double pos[3] = {double(row[0]), double(row[1]), double(row[2])};
    double r_passed = 0.0;
    if (gate_id > wr_gate % 4) {
        wr_gate = gate_id;
        if (gate_id >= 0 && gate_id < 4 && gate_id < io.num_gates) {   // (gate_id >= 0 bounds the load: C's % is negative for a negative wr_gate)
#pragma unroll
            for (int k = 0; k < 3; ++k) tgt[k] = double(row[12 + 4 * gate_id + k]);
        }
        r_passed = 5.0;
    }
    const double r_col = (newly && !fin) ? -1.0 : 0.0, r_lap = (newly && fin) ? 10.0 : 0.0;
    const double pxy = sqrt((tgt[0] - prv[0]) * (tgt[0] - prv[0]) + (tgt[1] - prv[1]) * (tgt[1] - prv[1]));
    const double cxy = sqrt((tgt[0] - pos[0]) * (tgt[0] - pos[0]) + (tgt[1] - pos[1]) * (tgt[1] - pos[1]));
    const double pz = fabs(tgt[2] - prv[2]), cz = fabs(tgt[2] - pos[2]);
    const double r = (pxy - cxy) + (pz - cz) + r_passed + r_col + r_lap;

    // selects, not products: a dead slot's row and a stale bootstrap value may hold anything
    const bool boot = was_alive && !done_now && tr && !te;
    const double stored = boot ? r + gamma * double(boot_value[j]) : r;
    rewards[j] = was_alive ? float(stored) : 0.0f;
    valid[j] = was_alive ? 1 : 0;
    next_start[j] = (done_now || te || tr) ? 1.0f : 0.0f;
    const bool ends = newly || (was_alive && (te || tr));
    const double ret = io.run_return[j] + r;
    const int len = io.run_length[j] + 1;
    ep_return[j] = ends ? ret : __builtin_nan("");
    ep_length[j] = ends ? len : 0;
    if (was_alive) {
        io.wr_gate[j] = wr_gate;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            io.wr_target[3 * j + k] = tgt[k];
            io.wr_prev[3 * j + k] = pos[k];
        }
        io.run_return[j] = ret;
        io.run_length[j] = len;
        io.alive[j] = done_now ? 0 : 1;
    }
}
