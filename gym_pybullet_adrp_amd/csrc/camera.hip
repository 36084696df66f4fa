// camera.hip — the drone camera of the race scene (include/adrp.h: adrp_race_camera, adrp_race_camera_env).
//
// The C-ABI around camera_kernel.h: what BaseAviary._getDroneImages renders per drone (BaseAviary.py:569-621),
// for E envs x N drones in one launch, by ray casting against the scene's analytic shapes (camera_core.h).
// Every refusal is made before the first device call, so it answers on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "adrp_internal.h"
#include "camera_kernel.h"

namespace {

// returns nullptr when the io's own fields are usable (the state pointers are the caller's to check)
const char* camera_io_error(const adrp_race_camera_io* io) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_race_camera_io)) return "adrp_race_camera_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->num_drones < 1 || io->num_drones > ADRP_MAX_DRONES) return "num_drones must be in 1..ADRP_MAX_DRONES";
    if (io->width < 1 || io->height < 1) return "width and height must be at least 1";
    // one workgroup of 256 lanes per (env, drone): HIP takes fewer than 2^32 lanes per launch
    if ((long long)io->num_envs * io->num_drones >= (1LL << 24)) return "num_envs * num_drones must be below 2^24";
    if ((long long)io->num_envs * io->num_drones * io->height > 0x7fffffffLL ||
        (long long)io->num_envs * io->num_drones * io->height * io->width > 0x7fffffffLL)
        return "num_envs * num_drones * height * width is past 2^31 - 1";
    if (!io->dep && !io->seg && !io->rgb) return "no output: dep, seg and rgb are all NULL";
    if (((uintptr_t)io->dep | (uintptr_t)io->seg | (uintptr_t)io->rgb) & 3u) return "dep, seg and rgb must be 4-byte aligned";
    if (io->capture_freq < 0) return "capture_freq must not be negative";
    return nullptr;
}

const char* camera_scene_error(const adrp_race_camera_io* io) {
    if (io->num_gates < 0 || io->num_gates > ADRP_MAX_GATES) return "num_gates must be in 0..ADRP_MAX_GATES";
    if (io->num_obstacles < 0 || io->num_obstacles > ADRP_MAX_OBSTACLES) return "num_obstacles must be in 0..ADRP_MAX_OBSTACLES";
    if (io->precision != 0 && io->precision != 1) return "precision must be 0 (float) or 1 (double)";
    if (!io->pos || !io->quat) return "NULL state pointer (pos / quat)";
    if (io->num_gates > 0 && !io->gates) return "NULL state pointer (gates)";
    if (io->num_obstacles > 0 && !io->obstacles) return "NULL state pointer (obstacles)";
    if (io->capture_freq > 0 && !io->step_counter) return "capture_freq > 0 needs step_counter";
    return nullptr;
}

template <typename Real>
int camera_launch(const adrp_race_camera_io* io, const int gate_low[4], int G, int O, const void* pos, const void* quat,
                  const void* gates, const void* obst, const int32_t* step_counter, hipStream_t s) {
    adrp_cam::CamArgs<Real> a;
    a.sc.N = io->num_drones; a.sc.G = G; a.sc.O = O;
    for (int g = 0; g < 4; ++g) a.sc.gate_low[g] = gate_low[g] != 0;
    a.sc.EN = size_t(io->num_envs) * io->num_drones;
    a.sc.pos = (const Real*)pos; a.sc.quat = (const Real*)quat;
    a.sc.gates = (const Real*)gates; a.sc.obst = (const Real*)obst;
    a.width = io->width; a.height = io->height;
    a.capture_freq = io->capture_freq;
    a.step_counter = step_counter;
    a.mask = io->mask;
    a.dep = io->dep; a.seg = io->seg; a.rgb = (uint32_t*)io->rgb;
    hipLaunchKernelGGL(adrp_cam::race_camera_kernel<Real>, dim3(unsigned(a.sc.EN)), dim3(adrp_cam::kCamLanes), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("race camera launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}

}  // namespace

extern "C" int adrp_race_camera(const adrp_race_camera_io* io, void* stream) {
    const char* why = camera_io_error(io);
    if (!why) why = camera_scene_error(io);
    if (why) return seterr(nullptr, ADRP_ERR_INVALID, std::string("adrp_race_camera: ") + why);
    StreamDeviceGuard g((hipStream_t)stream);
    if (io->precision)
        return camera_launch<double>(io, io->gate_low, io->num_gates, io->num_obstacles, io->pos, io->quat, io->gates,
                                     io->obstacles, io->step_counter, (hipStream_t)stream);
    return camera_launch<float>(io, io->gate_low, io->num_gates, io->num_obstacles, io->pos, io->quat, io->gates,
                                io->obstacles, io->step_counter, (hipStream_t)stream);
}

extern "C" int adrp_race_camera_env(const adrp_race_camera_io* io, adrp_t* h, void* stream) {
    const char* why = camera_io_error(io);
    if (!why && !h) why = "handle is NULL";
    if (!why && h->pbox) why = "persistent mode is active (adrp_persistent_end first)";
    if (!why && h->cfg.task != ADRP_TASK_RACE) why = "not a MultiRaceAviary handle";
    if (!why && (io->num_envs != h->E || io->num_drones != h->N)) why = "num_envs / num_drones differ from the handle's";
    if (why) return seterr(nullptr, ADRP_ERR_INVALID, std::string("adrp_race_camera_env: ") + why);
    const adrp_track& t = h->cfg.track;
    int low[4] = {0, 0, 0, 0};
    for (int g = 0; g < t.num_gates && g < 4; ++g) low[g] = t.gates[g][6] > 0;
    const size_t EN = size_t(h->E) * h->N, rs = h->real_size;
    const char* f = (const char*)h->f;
    DeviceGuard g(h->device);
    const int32_t* sc = h->ist + size_t(RI_STEP) * EN;
    if (rs == 8)
        return camera_launch<double>(io, low, t.num_gates, t.num_obstacles, f + RF_POS * EN * rs, f + RF_QUAT * EN * rs,
                                     f + RF_GATE * EN * rs, f + RF_OBST * EN * rs, sc, (hipStream_t)stream);
    return camera_launch<float>(io, low, t.num_gates, t.num_obstacles, f + RF_POS * EN * rs, f + RF_QUAT * EN * rs,
                                f + RF_GATE * EN * rs, f + RF_OBST * EN * rs, sc, (hipStream_t)stream);
}
