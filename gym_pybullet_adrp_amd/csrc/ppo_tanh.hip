// ppo_tanh.hip — ppo_grad_kernel for Tanh policies (SB3's MlpPolicy default)
#include "ppo_launch.h"

namespace adrp {
hipError_t ppo_grad_launch_tanh(int h1, int h2, const PpoGradArgs& a, int grid, hipStream_t s) {
    return ppo_grad_t1<false>(h1, h2, a, grid, s);
}
}  // namespace adrp
