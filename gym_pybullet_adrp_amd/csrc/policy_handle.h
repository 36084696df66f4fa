// policy_handle.h — the host object behind adrp_policy_t (policy.hip owns it; ppo.hip's learner
// rewrites its device blobs in place).
#pragma once

#include "policy_kernel.h"

struct adrp_policy {
    int device = 0;
    int in_dim = 0, h1 = 0, h2 = 0, relu = 0, act_dim = 4;
    int row_tiles = 0;       // 16-row tiles per block (ADRP_POLICY_RT; 0 = default)
    int wide = 0;            // served by the wide kernels: in_dim > 64, act_dim > 4 or ADRP_POLICY_WIDE=1
    adrp::PolicyLayout L{};
    float* blob = nullptr;   // device fragment blob
    adrp::PolicyLayout Lc{}; // critic (adrp_policy_set_critic)
    float* critic = nullptr;
    float* log_std = nullptr;
};
