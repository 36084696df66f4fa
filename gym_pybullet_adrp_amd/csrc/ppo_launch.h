// ppo_launch.h — the T1 x T2 instantiations of ppo_grad_kernel for one activation; included by
// ppo_tanh.hip / ppo_relu.hip (two translation units, so that they compile in parallel).
#pragma once

#include "ppo_kernel.h"

namespace adrp {

template <int T1, int T2, bool RELU>
static hipError_t ppo_grad_go(const PpoGradArgs& a, int grid, hipStream_t s) {
    constexpr int NW = T1 > T2 ? T1 : T2;
    hipLaunchKernelGGL((ppo_grad_kernel<T1, T2, RELU>), dim3(grid), dim3(128 * NW), 0, s, a);
    return hipGetLastError();
}

template <int T1, bool RELU>
static hipError_t ppo_grad_t2(int h2, const PpoGradArgs& a, int grid, hipStream_t s) {
    switch (h2 / 16) {
        case 1: return ppo_grad_go<T1, 1, RELU>(a, grid, s);
        case 2: return ppo_grad_go<T1, 2, RELU>(a, grid, s);
        case 4: return ppo_grad_go<T1, 4, RELU>(a, grid, s);
        default: return ppo_grad_go<T1, 8, RELU>(a, grid, s);
    }
}

template <bool RELU>
static hipError_t ppo_grad_t1(int h1, int h2, const PpoGradArgs& a, int grid, hipStream_t s) {
    switch (h1 / 16) {
        case 1: return ppo_grad_t2<1, RELU>(h2, a, grid, s);
        case 2: return ppo_grad_t2<2, RELU>(h2, a, grid, s);
        case 4: return ppo_grad_t2<4, RELU>(h2, a, grid, s);
        default: return ppo_grad_t2<8, RELU>(h2, a, grid, s);
    }
}

}  // namespace adrp
