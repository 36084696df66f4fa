// race_host_checks.h — the host-side refusals and launch plumbing that agents.hip and roster.hip share (and, where
// it is the same for its own io types, sim.hip): the adrp_race_agents_io validator, the NULL checks of the step
// entry points' arguments, the handle checks of the *_step_env forms, the launch-error answer.
//
// Every check returns the reason as a string (nullptr: nothing to refuse) and makes no device call; the entry point
// puts its own name in front with refuse().
#pragma once

#include <stdint.h>

#include <string>

#include "adrp_internal.h"

inline int refuse(const char* fn, const std::string& why) { return seterr(nullptr, ADRP_ERR_INVALID, std::string(fn) + ": " + why); }

// after a kernel launch: ADRP_OK, or the launch's error as "<what> launch: <HIP's text>"
inline int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string(what) + " launch: " + hipGetErrorString(e));
    return ADRP_OK;
}

// the race state's int image: field k of drone slot e * N + n at ist[k * E * N + e * N + n] (RaceInt)
inline const int32_t* race_int_field(const adrp_t* h, int k) { return h->ist + size_t(k) * h->E * h->N; }

// returns nullptr when io is usable
inline const char* agents_io_error(const adrp_race_agents_io* io) {
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

inline const char* step_outputs_error(const float* rewards, const uint8_t* valid, const float* next_start, const double* ep_return,
                                      const int32_t* ep_length) {
    if (!rewards || !valid || !next_start || !ep_return || !ep_length)
        return "NULL output (rewards / valid / next_start / ep_return / ep_length)";
    return nullptr;
}

// the step from caller arrays (adrp_race_agents_step, adrp_race_roster_step)
inline const char* step_args_error(const float* obs, const int32_t* gate, const int32_t* flags, const uint8_t* term,
                                   const uint8_t* trunc, const float* boot_value, const float* rewards, const uint8_t* valid,
                                   const float* next_start, const double* ep_return, const int32_t* ep_length) {
    if (!obs || !gate || !flags || !term || !trunc || !boot_value)
        return "NULL argument (obs / gate / flags / term / trunc / boot_value)";
    return step_outputs_error(rewards, valid, next_start, ep_return, ep_length);
}

// the step that reads gate / flags from an env handle (the *_step_env forms): the handle against the agents io,
// then the arguments
inline const char* step_env_args_error(const adrp_t* h, const adrp_race_agents_io* io, const float* obs, const uint8_t* term,
                                       const uint8_t* trunc, const float* boot_value, const float* rewards, const uint8_t* valid,
                                       const float* next_start, const double* ep_return, const int32_t* ep_length) {
    if (!h) return "the handle is NULL";
    if (h->cfg.task != ADRP_TASK_RACE) return "not a MultiRaceAviary handle";
    if (h->E != io->num_envs || h->N != io->num_drones || h->D != io->obs_dim) return "the handle's E, N, D differ from the io's";
    if (!obs || !term || !trunc || !boot_value) return "NULL argument (obs / term / trunc / boot_value)";
    return step_outputs_error(rewards, valid, next_start, ep_return, ep_length);
}
