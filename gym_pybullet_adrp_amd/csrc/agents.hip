// agents.hip — per-drone PPO agents of a multi-drone race (include/adrp.h: adrp_race_agents_*).
//
// The C-ABI around agents_kernel.h: one small launch per env.step next to the race step, one per masked reset.
// Every refusal is made before the first device call, so it answers on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "adrp_internal.h"
#include "agents_kernel.h"

namespace {

int agents_err(const char* fn, const std::string& why) { return seterr(nullptr, ADRP_ERR_INVALID, std::string(fn) + ": " + why); }

// returns nullptr when io is usable
const char* agents_io_error(const adrp_race_agents_io* io) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_race_agents_io)) return "adrp_race_agents_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->num_drones < 1 || io->num_drones > ADRP_MAX_DRONES) return "num_drones must be in 1..ADRP_MAX_DRONES";
    if (io->obs_dim < ADRP_AGENTS_OBS_MIN) return "obs_dim must be at least 49 (the gate id is column 48)";
    if (io->num_gates < 0 || io->num_gates > ADRP_MAX_GATES) return "num_gates must be in 0..ADRP_MAX_GATES";
    if ((long long)io->num_envs * io->num_drones * io->obs_dim > 0x7fffffffLL) return "num_envs * num_drones * obs_dim is too large";
    if (!io->wr_gate || !io->wr_target || !io->wr_prev || !io->alive || !io->run_return || !io->run_length)
        return "NULL buffer in adrp_race_agents_io";
    return nullptr;
}

int agents_grid(const adrp_race_agents_io* io) { return (io->num_envs * io->num_drones + kAgentLanes - 1) / kAgentLanes; }

int step_launch(const adrp_race_agents_io* io, const float* obs, const int32_t* gate, const int32_t* flags, const uint8_t* term,
                const uint8_t* trunc, const float* boot_value, double gamma, float* rewards, uint8_t* valid,
                float* next_start, double* ep_return, int32_t* ep_length, hipStream_t s) {
    hipLaunchKernelGGL(race_agents_step_kernel, dim3(agents_grid(io)), dim3(kAgentLanes), 0, s, *io, obs, gate, flags, term,
                       trunc, boot_value, gamma, rewards, valid, next_start, ep_return, ep_length);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("race agents step launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}

}  // namespace

extern "C" int adrp_race_agents_reset(const adrp_race_agents_io* io, const float* obs, const uint8_t* mask, void* stream) {
    if (const char* why = agents_io_error(io)) return agents_err("adrp_race_agents_reset", why);
    if (!obs) return agents_err("adrp_race_agents_reset", "NULL argument (obs)");
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(race_agents_reset_kernel, dim3(agents_grid(io)), dim3(kAgentLanes), 0, (hipStream_t)stream, *io, obs, mask);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("race agents reset launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}

extern "C" int adrp_race_agents_step(const adrp_race_agents_io* io, const float* obs, const int32_t* gate, const int32_t* flags,
                                     const uint8_t* term, const uint8_t* trunc, const float* boot_value, double gamma,
                                     float* rewards, uint8_t* valid, float* next_start, double* ep_return,
                                     int32_t* ep_length, void* stream) {
    if (const char* why = agents_io_error(io)) return agents_err("adrp_race_agents_step", why);
    if (!obs || !gate || !flags || !term || !trunc || !boot_value)
        return agents_err("adrp_race_agents_step", "NULL argument (obs / gate / flags / term / trunc / boot_value)");
    if (!rewards || !valid || !next_start || !ep_return || !ep_length)
        return agents_err("adrp_race_agents_step", "NULL output (rewards / valid / next_start / ep_return / ep_length)");
    StreamDeviceGuard g((hipStream_t)stream);
    return step_launch(io, obs, gate, flags, term, trunc, boot_value, gamma, rewards, valid, next_start, ep_return, ep_length,
                       (hipStream_t)stream);
}

extern "C" int adrp_race_agents_step_env(const adrp_race_agents_io* io, adrp_t* h, const float* obs, const uint8_t* term,
                                         const uint8_t* trunc, const float* boot_value, double gamma, float* rewards,
                                         uint8_t* valid, float* next_start, double* ep_return, int32_t* ep_length,
                                         void* stream) {
    if (const char* why = agents_io_error(io)) return agents_err("adrp_race_agents_step_env", why);
    if (!h) return agents_err("adrp_race_agents_step_env", "the handle is NULL");
    if (h->cfg.task != ADRP_TASK_RACE) return agents_err("adrp_race_agents_step_env", "not a MultiRaceAviary handle");
    if (h->E != io->num_envs || h->N != io->num_drones || h->D != io->obs_dim)
        return agents_err("adrp_race_agents_step_env", "the handle's E, N, D differ from the io's");
    if (!obs || !term || !trunc || !boot_value)
        return agents_err("adrp_race_agents_step_env", "NULL argument (obs / term / trunc / boot_value)");
    if (!rewards || !valid || !next_start || !ep_return || !ep_length)
        return agents_err("adrp_race_agents_step_env", "NULL output (rewards / valid / next_start / ep_return / ep_length)");
    // the race state's int image: field k of drone slot e * N + n at ist[k * E * N + e * N + n] (RaceInt)
    const size_t EN = size_t(h->E) * h->N;
    DeviceGuard g(h->device);
    return step_launch(io, obs, h->ist + size_t(RI_GATE) * EN, h->ist + size_t(RI_FLAGS) * EN, term, trunc, boot_value, gamma,
                       rewards, valid, next_start, ep_return, ep_length, (hipStream_t)stream);
}
