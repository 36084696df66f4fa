// ppo_relu.hip — ppo_grad_kernel for ReLU policies (policy_kwargs activation_fn=nn.ReLU)
#include "ppo_launch.h"

namespace adrp {
hipError_t ppo_grad_launch_relu(int h1, int h2, const PpoGradArgs& a, int grid, hipStream_t s) {
    return ppo_grad_t1<true>(h1, h2, a, grid, s);
}
}  // namespace adrp
