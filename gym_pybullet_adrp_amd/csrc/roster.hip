// roster.hip — race rosters for per-drone PPO rollouts (include/adrp.h: adrp_race_roster_*).
//
// The C-ABI around roster_kernel.h: three small launches per env.step of a RosterRolloutCollector (the command
// rows before the step, the learner columns' bookkeeping after it, the per-env clocks after the masked reset).
// Every refusal is made before the first device call, so it answers on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "adrp_internal.h"
#include "race_host_checks.h"
#include "roster_kernel.h"

namespace {

// the roster itself (sizes, roles, learner_index): returns nullptr when usable; who: learner l -> its drone
const char* roster_error(const adrp_race_roster_io* io, RosterLearners* who) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_race_roster_io)) return "adrp_race_roster_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->num_drones < 1 || io->num_drones > ADRP_MAX_DRONES) return "num_drones must be in 1..ADRP_MAX_DRONES";
    if (io->num_learners < 1 || io->num_learners > io->num_drones) return "num_learners must be in 1..num_drones";
    if ((long long)io->num_envs * io->num_drones > 0x7fffffffLL / ADRP_CMD_ARGS) return "num_envs * num_drones is too large";
    for (int l = 0; l < ADRP_MAX_DRONES; ++l) who->drone[l] = -1;
    int learners = 0;
    for (int n = 0; n < io->num_drones; ++n) {
        const int r = io->role[n], l = io->learner_index[n];
        if (r != ADRP_ROSTER_NONE && r != ADRP_ROSTER_HARDCODED && r != ADRP_ROSTER_POLICY && r != ADRP_ROSTER_LEARNER)
            return "role must be ADRP_ROSTER_NONE, _HARDCODED, _POLICY or _LEARNER";
        if (r != ADRP_ROSTER_LEARNER) {
            if (l >= 0) return "learner_index must be -1 on a drone that is not a LEARNER";
            continue;
        }
        learners += 1;
        if (l < 0 || l >= io->num_learners) return "learner_index of a LEARNER drone must be in 0..num_learners-1";
        if (who->drone[l] >= 0) return "learner_index gives two LEARNER drones the same index";
        who->drone[l] = n;
    }
    if (learners != io->num_learners) return "learner_index: the number of LEARNER drones is not num_learners";
    return nullptr;
}

// what the act and tick launches need on top of the roster
const char* buffers_error(const adrp_race_roster_io* io) {
    if (!(io->ctrl_freq > 0.0)) return "ctrl_freq must be positive";
    if (!io->clock || !io->phase || !io->codes || !io->args) return "NULL buffer in adrp_race_roster_io (clock / phase / codes / args)";
    if (reinterpret_cast<uintptr_t>(io->args) & 15) return "args must be 16-byte aligned";
    for (int n = 0; n < io->num_drones; ++n) {
        const int r = io->role[n];
        if (r == ADRP_ROSTER_HARDCODED && (!io->ref || !io->offset || io->ref_len < 1))
            return "a HARDCODED drone needs the ref table (ref, offset, ref_len >= 1)";
        if (r == ADRP_ROSTER_POLICY && !io->setpoints) return "a POLICY drone needs the setpoints buffer";
        if (r == ADRP_ROSTER_POLICY && (reinterpret_cast<uintptr_t>(io->setpoints) & 15)) return "setpoints must be 16-byte aligned";
        if (r == ADRP_ROSTER_LEARNER && !io->learner_act) return "a LEARNER drone needs the learner_act buffer";
        if (r == ADRP_ROSTER_LEARNER && (reinterpret_cast<uintptr_t>(io->learner_act) & 15))
            return "learner_act must be 16-byte aligned";
    }
    return nullptr;
}

// the agents io of the compact step: in the roster's shape (asked once its struct_size says the fields are there), and
// usable by agents.hip's checks
const char* agents_error(const adrp_race_roster_io* io, const adrp_race_agents_io* ag) {
    if (!ag) return "the agents io is NULL";
    if (ag->struct_size == sizeof(adrp_race_agents_io) && (ag->num_envs != io->num_envs || ag->num_drones != io->num_drones))
        return "the agents io's num_envs, num_drones differ from the roster's";
    return agents_io_error(ag);
}

int slot_grid(const adrp_race_roster_io* io) { return (io->num_envs * io->num_drones + kRosterLanes - 1) / kRosterLanes; }

int step_launch(const adrp_race_roster_io* io, const RosterLearners& who, const adrp_race_agents_io* ag, const float* obs,
                const int32_t* gate, const int32_t* flags, const uint8_t* term, const uint8_t* trunc, const float* boot_value,
                double gamma, float* rewards, uint8_t* valid, float* next_start, double* ep_return, int32_t* ep_length,
                hipStream_t s) {
    const int cols = io->num_learners * io->num_envs;
    hipLaunchKernelGGL(race_roster_step_kernel, dim3((cols + kRosterLanes - 1) / kRosterLanes), dim3(kRosterLanes), 0, s, *ag, who,
                       io->num_learners, obs, gate, flags, term, trunc, boot_value, gamma, rewards, valid, next_start, ep_return,
                       ep_length);
    return launched("race roster step");
}

}  // namespace

extern "C" int adrp_race_roster_act(const adrp_race_roster_io* io, void* stream) {
    RosterLearners who;
    if (const char* why = roster_error(io, &who)) return refuse("adrp_race_roster_act", why);
    if (const char* why = buffers_error(io)) return refuse("adrp_race_roster_act", why);
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(race_roster_act_kernel, dim3(slot_grid(io)), dim3(kRosterLanes), 0, (hipStream_t)stream, *io);
    return launched("race roster act");
}

extern "C" int adrp_race_roster_tick(const adrp_race_roster_io* io, const uint8_t* mask, void* stream) {
    RosterLearners who;
    if (const char* why = roster_error(io, &who)) return refuse("adrp_race_roster_tick", why);
    if (const char* why = buffers_error(io)) return refuse("adrp_race_roster_tick", why);
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(race_roster_tick_kernel, dim3(slot_grid(io)), dim3(kRosterLanes), 0, (hipStream_t)stream, *io, mask);
    return launched("race roster tick");
}

extern "C" int adrp_race_roster_step(const adrp_race_roster_io* io, const adrp_race_agents_io* agents, const float* obs,
                                     const int32_t* gate, const int32_t* flags, const uint8_t* term, const uint8_t* trunc,
                                     const float* boot_value, double gamma, float* rewards, uint8_t* valid, float* next_start,
                                     double* ep_return, int32_t* ep_length, void* stream) {
    RosterLearners who;
    if (const char* why = roster_error(io, &who)) return refuse("adrp_race_roster_step", why);
    if (const char* why = agents_error(io, agents)) return refuse("adrp_race_roster_step", why);
    if (const char* why = step_args_error(obs, gate, flags, term, trunc, boot_value, rewards, valid, next_start, ep_return, ep_length))
        return refuse("adrp_race_roster_step", why);
    StreamDeviceGuard g((hipStream_t)stream);
    return step_launch(io, who, agents, obs, gate, flags, term, trunc, boot_value, gamma, rewards, valid, next_start, ep_return,
                       ep_length, (hipStream_t)stream);
}

extern "C" int adrp_race_roster_done(const adrp_race_roster_io* io, const adrp_race_agents_io* agents, const uint8_t* term,
                                     const uint8_t* trunc, uint8_t* mask_out, void* stream) {
    RosterLearners who;
    if (const char* why = roster_error(io, &who)) return refuse("adrp_race_roster_done", why);
    if (const char* why = agents_error(io, agents)) return refuse("adrp_race_roster_done", why);
    if (!term || !trunc || !mask_out) return refuse("adrp_race_roster_done", "NULL argument (term / trunc / mask_out)");
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(race_roster_done_kernel, dim3((io->num_envs + kRosterLanes - 1) / kRosterLanes), dim3(kRosterLanes), 0,
                       (hipStream_t)stream, io->num_envs, io->num_drones, who, io->num_learners, agents->alive, term, trunc,
                       mask_out);
    return launched("race roster done");
}

extern "C" int adrp_race_roster_step_env(const adrp_race_roster_io* io, const adrp_race_agents_io* agents, adrp_t* h,
                                         const float* obs, const uint8_t* term, const uint8_t* trunc, const float* boot_value,
                                         double gamma, float* rewards, uint8_t* valid, float* next_start, double* ep_return,
                                         int32_t* ep_length, void* stream) {
    RosterLearners who;
    if (const char* why = roster_error(io, &who)) return refuse("adrp_race_roster_step_env", why);
    if (const char* why = agents_error(io, agents)) return refuse("adrp_race_roster_step_env", why);
    if (const char* why = step_env_args_error(h, agents, obs, term, trunc, boot_value, rewards, valid, next_start, ep_return,
                                              ep_length))
        return refuse("adrp_race_roster_step_env", why);
    DeviceGuard g(h->device);
    return step_launch(io, who, agents, obs, race_int_field(h, RI_GATE), race_int_field(h, RI_FLAGS), term, trunc, boot_value,
                       gamma, rewards, valid, next_start, ep_return, ep_length, (hipStream_t)stream);
}
