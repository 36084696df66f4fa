// policy_wide.hip — the wide policy kernels' instantiations and launchers (policy_kernel.h:
// policy_wide_kernel / policy_sample_wide_kernel; in_dim <= 576, act_dim <= 32).  Their own
// translation unit: T1 x T2 x RELU is 32 instantiations per kernel, compiled beside policy.hip.
#include <hip/hip_runtime.h>

#include "policy_kernel.h"

namespace adrp {

template <int T1, int T2>
static hipError_t launch_act(const float* blob, const PolicyLayout& L, int relu, const float* obs, int rows, int stride,
                             float* act, int mode, hipStream_t s) {
    const dim3 grid((rows + 15) / 16), blk(64 * (T1 > T2 ? T1 : T2));
    if (relu) hipLaunchKernelGGL((policy_wide_kernel<T1, T2, true>), grid, blk, 0, s, blob, L, obs, rows, stride, act, mode);
    else hipLaunchKernelGGL((policy_wide_kernel<T1, T2, false>), grid, blk, 0, s, blob, L, obs, rows, stride, act, mode);
    return hipGetLastError();
}

template <int T1>
static hipError_t act_t2(const float* blob, const PolicyLayout& L, int h2, int relu, const float* obs, int rows, int stride,
                         float* act, int mode, hipStream_t s) {
    switch (h2 / 16) {
        case 1: return launch_act<T1, 1>(blob, L, relu, obs, rows, stride, act, mode, s);
        case 2: return launch_act<T1, 2>(blob, L, relu, obs, rows, stride, act, mode, s);
        case 4: return launch_act<T1, 4>(blob, L, relu, obs, rows, stride, act, mode, s);
        default: return launch_act<T1, 8>(blob, L, relu, obs, rows, stride, act, mode, s);
    }
}

hipError_t policy_wide_launch(const float* blob, const PolicyLayout& L, int h1, int h2, int relu, const float* obs, int rows,
                              int obs_stride, float* act, int mode, hipStream_t s) {
    switch (h1 / 16) {
        case 1: return act_t2<1>(blob, L, h2, relu, obs, rows, obs_stride, act, mode, s);
        case 2: return act_t2<2>(blob, L, h2, relu, obs, rows, obs_stride, act, mode, s);
        case 4: return act_t2<4>(blob, L, h2, relu, obs, rows, obs_stride, act, mode, s);
        default: return act_t2<8>(blob, L, h2, relu, obs, rows, obs_stride, act, mode, s);
    }
}

template <int T1, int T2>
static hipError_t launch_sample(int relu, const PolicySampleArgs& a, hipStream_t s) {
    constexpr int NW = T1 > T2 ? T1 : T2;
    const dim3 grid((a.rows + 15) / 16), blk(2 * 64 * NW);
    if (relu) hipLaunchKernelGGL((policy_sample_wide_kernel<T1, T2, true>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((policy_sample_wide_kernel<T1, T2, false>), grid, blk, 0, s, a);
    return hipGetLastError();
}

template <int T1>
static hipError_t sample_t2(int h2, int relu, const PolicySampleArgs& a, hipStream_t s) {
    switch (h2 / 16) {
        case 1: return launch_sample<T1, 1>(relu, a, s);
        case 2: return launch_sample<T1, 2>(relu, a, s);
        case 4: return launch_sample<T1, 4>(relu, a, s);
        default: return launch_sample<T1, 8>(relu, a, s);
    }
}

hipError_t policy_sample_wide_launch(int h1, int h2, int relu, const PolicySampleArgs& a, hipStream_t s) {
    switch (h1 / 16) {
        case 1: return sample_t2<1>(h2, relu, a, s);
        case 2: return sample_t2<2>(h2, relu, a, s);
        case 4: return sample_t2<4>(h2, relu, a, s);
        default: return sample_t2<8>(h2, relu, a, s);
    }
}

}  // namespace adrp
