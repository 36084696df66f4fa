// plan.hip — the scripted racer's device spline planner (include/adrp.h: adrp_race_plan).
//
// The C-ABI around plan_kernel.h: what HardCodedController.__init__ does per drone at every episode start
// (user_controller/HardCodedController.py:63-115: waypoints, splprep, splev), for E envs x N drones in one launch.
// Every refusal is made before the first device call, so it answers on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "adrp_internal.h"
#include "plan_kernel.h"

namespace {

// returns nullptr when io is usable
const char* plan_io_error(const adrp_race_plan_io* io) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_race_plan_io)) return "adrp_race_plan_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->num_drones < 1 || io->num_drones > ADRP_MAX_DRONES) return "num_drones must be in 1..ADRP_MAX_DRONES";
    if (io->ref_len < 2) return "ref_len must be at least 2";
    if (io->obs_stride < ADRP_PLAN_OBS_MIN) return "obs_stride must be at least 28 (the start in [0:2], the gates in [12:28])";
    if ((long long)io->num_envs * io->num_drones > 0x7fffffffLL) return "num_envs * num_drones is too large";
    if (!io->obs || !io->samples || !io->ref || !io->status) return "NULL buffer in adrp_race_plan_io (obs / samples / ref / status)";
    return nullptr;
}

}  // namespace

extern "C" int adrp_race_plan(const adrp_race_plan_io* io, void* stream) {
    if (const char* why = plan_io_error(io)) return seterr(nullptr, ADRP_ERR_INVALID, std::string("adrp_race_plan: ") + why);
    StreamDeviceGuard g((hipStream_t)stream);
    const long long EN = (long long)io->num_envs * io->num_drones;
    const unsigned blocks = unsigned((EN + kPlanLanes - 1) / kPlanLanes);
    hipLaunchKernelGGL(race_plan_kernel, dim3(blocks), dim3(kPlanLanes), 0, (hipStream_t)stream, *io);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("race plan launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}
