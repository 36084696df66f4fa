// agents.hip — per-drone PPO agents of a multi-drone race (include/adrp.h: adrp_race_agents_*).
//
// The C-ABI around agents_kernel.h: one small launch per env.step next to the race step, one per masked reset.
// Every refusal is made before the first device call, so it answers on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "adrp_internal.h"
#include "agents_kernel.h"
#include "race_host_checks.h"

namespace {

int agents_grid(const adrp_race_agents_io* io) { return (io->num_envs * io->num_drones + kAgentLanes - 1) / kAgentLanes; }

int step_launch(const adrp_race_agents_io* io, const float* obs, const int32_t* gate, const int32_t* flags, const uint8_t* term,
                const uint8_t* trunc, const float* boot_value, double gamma, float* rewards, uint8_t* valid,
                float* next_start, double* ep_return, int32_t* ep_length, hipStream_t s) {
    hipLaunchKernelGGL(race_agents_step_kernel, dim3(agents_grid(io)), dim3(kAgentLanes), 0, s, *io, obs, gate, flags, term,
                       trunc, boot_value, gamma, rewards, valid, next_start, ep_return, ep_length);
    return launched("race agents step");
}

}  // namespace

extern "C" int adrp_race_agents_reset(const adrp_race_agents_io* io, const float* obs, const uint8_t* mask, void* stream) {
    if (const char* why = agents_io_error(io)) return refuse("adrp_race_agents_reset", why);
    if (!obs) return refuse("adrp_race_agents_reset", "NULL argument (obs)");
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(race_agents_reset_kernel, dim3(agents_grid(io)), dim3(kAgentLanes), 0, (hipStream_t)stream, *io, obs, mask);
    return launched("race agents reset");
}

extern "C" int adrp_race_agents_step(const adrp_race_agents_io* io, const float* obs, const int32_t* gate, const int32_t* flags,
                                     const uint8_t* term, const uint8_t* trunc, const float* boot_value, double gamma,
                                     float* rewards, uint8_t* valid, float* next_start, double* ep_return,
                                     int32_t* ep_length, void* stream) {
    if (const char* why = agents_io_error(io)) return refuse("adrp_race_agents_step", why);
    if (const char* why = step_args_error(obs, gate, flags, term, trunc, boot_value, rewards, valid, next_start, ep_return, ep_length))
        return refuse("adrp_race_agents_step", why);
    StreamDeviceGuard g((hipStream_t)stream);
    return step_launch(io, obs, gate, flags, term, trunc, boot_value, gamma, rewards, valid, next_start, ep_return, ep_length,
                       (hipStream_t)stream);
}

extern "C" int adrp_race_agents_step_env(const adrp_race_agents_io* io, adrp_t* h, const float* obs, const uint8_t* term,
                                         const uint8_t* trunc, const float* boot_value, double gamma, float* rewards,
                                         uint8_t* valid, float* next_start, double* ep_return, int32_t* ep_length,
                                         void* stream) {
    if (const char* why = agents_io_error(io)) return refuse("adrp_race_agents_step_env", why);
    if (const char* why = step_env_args_error(h, io, obs, term, trunc, boot_value, rewards, valid, next_start, ep_return, ep_length))
        return refuse("adrp_race_agents_step_env", why);
    DeviceGuard g(h->device);
    return step_launch(io, obs, race_int_field(h, RI_GATE), race_int_field(h, RI_FLAGS), term, trunc, boot_value, gamma,
                       rewards, valid, next_start, ep_return, ep_length, (hipStream_t)stream);
}
