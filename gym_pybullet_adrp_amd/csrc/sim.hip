// sim.hip — batched race evaluation (include/adrp.h: adrp_race_controllers / adrp_race_results_*).
//
// The C-ABI around sim_kernel.h: what scripts/sim.py:68-108 does per env.step next to env.step itself (the
// agents' predict calls, the reward sum, the episode-end test), for E envs x N drones in two small launches.
// Every refusal is made before the first device call, so it answers on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "adrp_internal.h"
#include "race_host_checks.h"
#include "sim_kernel.h"

namespace {

// returns nullptr when io is usable
const char* ctrl_io_error(const adrp_race_ctrl_io* io) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_race_ctrl_io)) return "adrp_race_ctrl_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->num_drones < 1 || io->num_drones > ADRP_MAX_DRONES) return "num_drones must be in 1..ADRP_MAX_DRONES";
    if ((long long)io->num_envs * io->num_drones > 0x7fffffffLL / ADRP_CMD_ARGS) return "num_envs * num_drones is too large";
    if (!io->codes || !io->args) return "NULL buffer in adrp_race_ctrl_io (codes / args)";
    if (reinterpret_cast<uintptr_t>(io->args) & 15) return "args must be 16-byte aligned";
    for (int n = 0; n < io->num_drones; ++n) {
        const int k = io->kind[n];
        if (k != ADRP_RACE_CTRL_NONE && k != ADRP_RACE_CTRL_HARDCODED && k != ADRP_RACE_CTRL_POLICY)
            return "kind must be ADRP_RACE_CTRL_NONE, _HARDCODED or _POLICY";
        if (k == ADRP_RACE_CTRL_HARDCODED && (!io->ref || !io->offset || !io->phase || io->ref_len < 1))
            return "a HARDCODED drone needs the ref table (ref, offset, phase, ref_len >= 1)";
        if (k == ADRP_RACE_CTRL_POLICY && !io->setpoints) return "a POLICY drone needs the setpoints buffer";
        if (k == ADRP_RACE_CTRL_POLICY && (reinterpret_cast<uintptr_t>(io->setpoints) & 15))
            return "setpoints must be 16-byte aligned";
    }
    return nullptr;
}

const char* results_io_error(const adrp_race_results_io* io) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_race_results_io)) return "adrp_race_results_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->num_drones < 1 || io->num_drones > ADRP_MAX_DRONES) return "num_drones must be in 1..ADRP_MAX_DRONES";
    if (io->capacity < 1) return "capacity must be at least 1";
    if ((long long)io->num_envs * io->num_drones > 0x7fffffffLL || (long long)io->capacity * io->num_drones > 0x7fffffffLL)
        return "num_envs / capacity x num_drones is too large";
    if (!io->open || !io->run_return || !io->run_length || !io->gates || !io->finish || !io->elim || !io->meta ||
        !io->log_return || !io->log_length || !io->log_term || !io->log_trunc || !io->log_gates || !io->log_finish ||
        !io->log_elim)
        return "NULL buffer in adrp_race_results_io";
    return nullptr;
}

const char* wave_error(const adrp_race_results_io* io, int base, int n_open) {
    if (n_open < 0 || n_open > io->num_envs) return "n_open must be in 0..num_envs";
    if (base < 0 || (long long)base + n_open > io->capacity) return "base + n_open exceeds the capacity";
    return nullptr;
}

int results_launch(const adrp_race_results_io* io, const int32_t* gate, const int32_t* flags,
                   const float* rew, const uint8_t* term, const uint8_t* trunc, hipStream_t s) {
    hipLaunchKernelGGL(race_results_kernel, dim3(1), dim3(kResLanes), 0, s, *io, gate, flags, rew, term, trunc);
    return launched("race results step");
}

}  // namespace

extern "C" int adrp_race_controllers(const adrp_race_ctrl_io* io, double ep_time, void* stream) {
    if (const char* why = ctrl_io_error(io)) return refuse("adrp_race_controllers", why);
    StreamDeviceGuard g((hipStream_t)stream);
    const int EN = io->num_envs * io->num_drones;
    hipLaunchKernelGGL(race_controller_kernel, dim3((EN + kCtrlLanes - 1) / kCtrlLanes), dim3(kCtrlLanes), 0,
                       (hipStream_t)stream, *io, ep_time);
    return launched("race controllers");
}

extern "C" int adrp_race_results_begin(adrp_race_results_io* io, int base, int n_open, void* stream) {
    if (const char* why = results_io_error(io)) return refuse("adrp_race_results_begin", why);
    if (const char* why = wave_error(io, base, n_open)) return refuse("adrp_race_results_begin", why);
    io->base = base;
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(race_results_begin_kernel, dim3(1), dim3(kResLanes), 0, (hipStream_t)stream, *io, n_open);
    return launched("race results begin");
}

extern "C" int adrp_race_results_step(const adrp_race_results_io* io, const int32_t* gate, const int32_t* flags,
                                      const float* rew, const uint8_t* term, const uint8_t* trunc, void* stream) {
    if (const char* why = results_io_error(io)) return refuse("adrp_race_results_step", why);
    if (const char* why = wave_error(io, io->base, 0)) return refuse("adrp_race_results_step", why);
    if (!gate || !flags || !rew || !term || !trunc)
        return refuse("adrp_race_results_step", "NULL argument (gate / flags / rew / term / trunc)");
    StreamDeviceGuard g((hipStream_t)stream);
    return results_launch(io, gate, flags, rew, term, trunc, (hipStream_t)stream);
}

extern "C" int adrp_race_results_step_env(const adrp_race_results_io* io, adrp_t* h, const float* rew, const uint8_t* term,
                                          const uint8_t* trunc, void* stream) {
    if (const char* why = results_io_error(io)) return refuse("adrp_race_results_step_env", why);
    if (const char* why = wave_error(io, io->base, 0)) return refuse("adrp_race_results_step_env", why);
    if (!h) return refuse("adrp_race_results_step_env", "the handle is NULL");
    if (h->cfg.task != ADRP_TASK_RACE) return refuse("adrp_race_results_step_env", "not a MultiRaceAviary handle");
    if (h->E != io->num_envs || h->N != io->num_drones)
        return refuse("adrp_race_results_step_env", "the handle's E, N differ from the io's");
    if (!rew || !term || !trunc) return refuse("adrp_race_results_step_env", "NULL argument (rew / term / trunc)");
    DeviceGuard g(h->device);
    return results_launch(io, race_int_field(h, RI_GATE), race_int_field(h, RI_FLAGS), rew, term, trunc, (hipStream_t)stream);
}
