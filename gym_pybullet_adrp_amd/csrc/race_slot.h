// race_slot.h — the per-slot bodies that the race evaluation, the per-drone agents and the roster collector share
// (sim_kernel.h race_controller_kernel, agents_kernel.h race_agents_step_kernel, roster_kernel.h): each is written
// once here and inlined into the kernels that call it, so two kernels fed the same inputs give the same bits.
// Plain loads, selects and vector stores; no LDS, no atomics.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/adrp.h"

namespace adrp {

constexpr double kHardCtrlFreq = 25.0;   // the scripted controller's own clock (utils/constants.py:31), not the env's

// One drone's command row at episode time ep_time: codes[slot] and the 14 doubles of args[slot], written whatever
// the kind.  kind: ADRP_RACE_CTRL_*; sp: this slot's setpoint (read for POLICY alone); phase uint8 [3][EN], ref
// [EN][L][3] and offset [EN] are read (and phase updated) for HARDCODED alone.
__device__ __forceinline__ void race_controller_slot(int slot, int EN, int kind, const float4* __restrict__ sp, int L,
                                                     const double* __restrict__ ref, const int64_t* __restrict__ offset,
                                                     uint8_t* __restrict__ phase, double ep_time,
                                                     int32_t* __restrict__ codes, double* __restrict__ args) {
    int code = ADRP_CMD_NONE;
    double a[ADRP_CMD_ARGS];
#pragma unroll
    for (int k = 0; k < ADRP_CMD_ARGS; ++k) a[k] = 0.0;
    if (kind == ADRP_RACE_CTRL_HARDCODED) {
        // HardCodedCommander.predict (hardcoded.py): step = clamp(int(ep_time * 25) - offset, 0, L)
        const long long it = (long long)__builtin_trunc(ep_time * kHardCtrlFreq);
        long long st = it - (long long)offset[slot];
        st = st < 0 ? 0 : (st > L ? L : st);
        const bool took = phase[slot] != 0, notified = phase[EN + slot] != 0, landed = phase[2 * EN + slot] != 0;
        const bool fst = took && st < L;
        const bool ntf = took && !fst && !notified;
        const bool lnd = took && !fst && notified && !landed;
        if (!took) {                       // TAKEOFF [0.3, 2]; the commander clock is args[-1] = 2
            code = ADRP_CMD_TAKEOFF;
            a[0] = 0.3; a[1] = 2.0; a[ADRP_CMD_TIME_SLOT] = 2.0;
            phase[slot] = 1;
        } else if (fst) {                  // FULLSTATE (ref[step], 0, 0.5 * ones(3), 0, 0, ep_time)
            const double* __restrict__ r = ref + (size_t(slot) * L + size_t(st)) * 3;
            code = ADRP_CMD_FULLSTATE;
            a[0] = r[0]; a[1] = r[1]; a[2] = r[2];
            a[6] = 0.5; a[7] = 0.5; a[8] = 0.5;
            a[ADRP_CMD_TIME_SLOT] = ep_time;
        } else if (ntf) {                  // NOTIFY [ep_time]
            code = ADRP_CMD_NOTIFY;
            a[0] = ep_time; a[ADRP_CMD_TIME_SLOT] = ep_time;
            phase[EN + slot] = 1;
        } else if (lnd) {                  // LAND [0, 2]
            code = ADRP_CMD_LAND;
            a[1] = 2.0; a[ADRP_CMD_TIME_SLOT] = 2.0;
            phase[2 * EN + slot] = 1;
        }
    } else if (kind == ADRP_RACE_CTRL_POLICY) {
        // RLController._action_transform: [action[:3], ZERO3, ZERO3, action[3], ZERO3, self.time]
        const float4 s = *sp;
        code = ADRP_CMD_FULLSTATE;
        a[0] = double(s.x); a[1] = double(s.y); a[2] = double(s.z);
        a[9] = double(s.w);
        a[ADRP_CMD_TIME_SLOT] = ep_time;
    }
    codes[slot] = code;
    double2* __restrict__ out = reinterpret_cast<double2*>(args + size_t(slot) * ADRP_CMD_ARGS);   // 112-byte rows
#pragma unroll
    for (int k = 0; k < ADRP_CMD_ARGS / 2; ++k) out[k] = make_double2(a[2 * k], a[2 * k + 1]);
}

// One agent's env.step: the state of slot j = e * N + n of io is read and updated, boot_value and the five outputs
// are indexed by the caller's column c (c = j in the full-width layout).  The reward's arithmetic is race_quad.h's
// drone-0 copy (oracle/race.c race_reward_wrapper) in float64 on the float32 row, with the drone's own "became
// done" / "finished" for terminated / task_completed.
__device__ __forceinline__ void race_agent_step_slot(const adrp_race_agents_io& io, int j, int e, int c,
                                                     const float* __restrict__ obs, const int32_t* __restrict__ gate,
                                                     const int32_t* __restrict__ flags, const uint8_t* __restrict__ term,
                                                     const uint8_t* __restrict__ trunc, const float* __restrict__ boot_value,
                                                     double gamma, float* __restrict__ rewards, uint8_t* __restrict__ valid,
                                                     float* __restrict__ next_start, double* __restrict__ ep_return,
                                                     int32_t* __restrict__ ep_length) {
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
    const double stored = boot ? r + gamma * double(boot_value[c]) : r;
    rewards[c] = was_alive ? float(stored) : 0.0f;
    valid[c] = was_alive ? 1 : 0;
    next_start[c] = (done_now || te || tr) ? 1.0f : 0.0f;
    const bool ends = newly || (was_alive && (te || tr));
    const double ret = io.run_return[j] + r;
    const int len = io.run_length[j] + 1;
    ep_return[c] = ends ? ret : __builtin_nan("");
    ep_length[c] = ends ? len : 0;
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

}  // namespace adrp
