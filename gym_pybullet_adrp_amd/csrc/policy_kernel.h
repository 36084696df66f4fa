// policy_kernel.h — fused on-device actor forward of an SB3 PPO MlpPolicy (two hidden layers)
// plus the RLController action transform, for closed-loop MultiRaceAviary rollouts with no
// host round-trip.
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   RLController.predict / _action_transform      user_controller/RLController.py:39-73
//   RLControllerTwoGates._action_transform        user_controller/RLControllerTwoGates.py:56-69
//   PPO.predict(obs, deterministic=True)          stable_baselines3 2.3.2 (the zips' version):
//     ActorCriticPolicy: Flatten -> mlp_extractor.policy_net (Linear, act, Linear, act)
//     -> action_net (Linear) = the Gaussian mean; BasePolicy.predict clips it to the Box [-1, 1]
//   map2pi                                        gym_pybullet_adrp/utils/utils.py:188-197
//
// Layout: one block = 16 observation rows; all three layers run on the f32-input MFMA
// v_mfma_f32_16x16x4_f32 (exact f32 fma chains, no reduced precision), oriented so that each
// layer's accumulator tile is, element for element, the next layer's B operand:
//   H1ᵀ = W1 · Xᵀ,  H2ᵀ = W2 · act(H1ᵀ + b1),  Oᵀ = W3 · act(H2ᵀ + b2)
// A 16x16 f32 accumulator holds [unit = 16 t + 4 (lane >> 4) + reg][row = lane & 15]; as a
// B operand, k-step (t, reg) then covers units {16 t + 4 g + reg : g = 0..3}.  The host
// pre-permutes every weight tile into that k order ("fragments": 64 floats, one per lane),
// so the hand-off between layers is a same-lane LDS store / load with no transpose.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adrp_device.h"

namespace adrp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// fragment-blob layout (floats), written by the host (policy.hip: build_blob).  Layer 1 is
// always kPolicyS1 = 16 k-steps (in_dim <= 64, zero-padded weights), so no loop has a
// runtime trip count.
constexpr int kPolicyS1 = 16;
// The wide kernels (below: policy_wide_kernel / policy_sample_wide_kernel) take layer 1 in chunks
// of kPolicyChunk k-steps (64 observation columns) with a runtime chunk count, and 1 or 2 output
// tiles.  kPolicyMaxIn = ADRP_MAX_DRONES (8) x 72, the widest joint MultiHoverAviary row at
// CTRL_FREQ 30 (12 + 15 x 4 floats per drone); raise it here (nothing else is sized by it).
constexpr int kPolicyChunk = 16;
constexpr int kPolicyMaxIn = 576;
constexpr int kPolicyMaxOut = 32;
struct PolicyLayout {
    int in_dim;              // observation width (<= 4 * s1)
    int f1, f2, f3;          // fragment offsets of layers 1..3 (in floats)
    int b1, b2, b3;          // bias offsets
    int total;               // blob size in floats
    int s1;                  // layer-1 k-steps in the blob: kPolicyS1 (narrow) or ceil(in_dim / 4) rounded up to
                             // a whole chunk (wide); fragment (t, s) at f1 + (t * s1 + s) * 64
    int t3;                  // output tiles = ceil(n_out / 16); fragment (u3, u, i) at f3 + ((u3 * T2 + u) * 4 + i) * 64,
                             // b3 holds 16 * t3 floats
    int n_out;               // live outputs (rows of W3); the rest of the last tile is zero
    int wide;                // 1: built for the wide kernels (s1 by in_dim), 0: the narrow layout (s1 = kPolicyS1)
};

// action transform (RLController._action_transform variants)
enum { POLICY_RAW = 0, POLICY_RELATIVE = 1, POLICY_ABSOLUTE = 2 };

// tanh(x) = (e^2x - 1) / (e^2x + 1), branch-free on the hardware exp2 / rcp (|x| clamped to 15,
// where tanh is 1 in f32); absolute error ~1e-7, far inside the policy's 2e-5 bar.  OCML's
// tanhf branches per lane range, which splits the unrolled MFMA schedule into blocks.
__device__ __forceinline__ float tanh_fast(float x) {
    const float c = __builtin_amdgcn_fmed3f(x, -15.0f, 15.0f);
    const float t = __builtin_amdgcn_exp2f(c * 2.8853900817779268f);     // e^(2c)
    return (t - 1.0f) * __builtin_amdgcn_rcpf(t + 1.0f);
}

template <bool RELU>
__device__ __forceinline__ float policy_act(float x) {
    if constexpr (RELU) return x > 0.0f ? x : 0.0f;
    else return tanh_fast(x);
}

// map2pi(angle) = ((angle + pi) % (2 pi)) - pi with NumPy's floor-mod, in float64
__device__ __forceinline__ double map2pi_d(double a) {
    const double two_pi = 6.283185307179586, pi = 3.141592653589793;
    const double x = a + pi;
    double r = fmod(x, two_pi);
    if (r != 0.0 && r < 0.0) r += two_pi;
    return r - pi;
}

// T1 = H1 / 16, T2 = H2 / 16, RELU (else Tanh).  One block = 16 observation rows and
// NW = max(T1, T2) waves: wave w owns hidden-unit tile w of each layer, so a launch has
// NW x rows / 16 waves (all SIMDs busy at the race batch sizes) and each wave issues its few
// weight fragments (read straight from global memory: 256 contiguous bytes per fragment per
// wave, the blob L2-resident after the first waves) together with its observation loads, at
// entry: one memory latency per launch.  The activations between layers go through LDS in
// the B-operand order, so every read and write is conflict-free (lds[(tile*4 + reg)*64 + lane]).
// RT row tiles (16 rows each) per block reuse the weight fragments a wave holds in registers.
template <int T1, int T2, bool RELU, int RT>
__global__ void __launch_bounds__(512) policy_kernel(const float* __restrict__ blob, PolicyLayout L,
                                                     const float* __restrict__ obs, int rows, int obs_stride,
                                                     float* __restrict__ act, int mode) {
    __shared__ float h1s[T1 * 4 * 64];
    __shared__ float h2s[T2 * 4 * 64];
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;          // wave = unit tile
    const int g = lane >> 4;
    const bool l1 = w < T1, l2 = w < T2;
    // ---- the weights this wave needs, issued up front, kept for all RT row tiles ----
    float w1f[kPolicyS1], w2f[T1][4], b1v[4], b2v[4];
#pragma unroll
    for (int s = 0; s < kPolicyS1; ++s) w1f[s] = blob[L.f1 + ((l1 ? w : 0) * kPolicyS1 + s) * 64 + lane];
#pragma unroll
    for (int t = 0; t < T1; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) w2f[t][i] = blob[L.f2 + (((l2 ? w : 0) * T1 + t) * 4 + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        b1v[i] = blob[L.b1 + 16 * (l1 ? w : 0) + 4 * g + i];
        b2v[i] = blob[L.b2 + 16 * (l2 ? w : 0) + 4 * g + i];
    }
    float w3f[T2][4], b3v[4];
    if (w == 0) {
#pragma unroll
        for (int u = 0; u < T2; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) w3f[u][i] = blob[L.f3 + (u * 4 + i) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) b3v[i] = blob[L.b3 + i];
    }
    for (int rt = 0; rt < RT; ++rt) {
    const int row0 = (blockIdx.x * RT + rt) * 16;
    if (row0 >= rows) return;                // block-uniform
    const int r = row0 + (lane & 15);
    const bool live = r < rows;
    const float* xrow = obs + size_t(live ? r : row0) * obs_stride;
    float xb[kPolicyS1];
#pragma unroll
    for (int s = 0; s < kPolicyS1; ++s) {
        const int k = 4 * s + g;
        const float v = xrow[k < L.in_dim ? k : 0];
        xb[s] = (live && k < L.in_dim) ? v : 0.0f;
    }

    // ---- layer 1, unit tile w: two interleaved accumulator chains over the 16 k-steps ----
    if (l1) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int s = 0; s < kPolicyS1; s += 2) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1f[s], xb[s], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1f[s + 1], xb[s + 1], a1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) h1s[(w * 4 + i) * 64 + lane] = policy_act<RELU>(a0[i] + a1[i] + b1v[i]);
    }
    __syncthreads();
    // ---- layer 2, unit tile w: B operands = layer-1 tiles (t, reg) from LDS ----
    if (l2) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int t = 0; t < T1; ++t)
#pragma unroll
            for (int i = 0; i < 4; i += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2f[t][i], h1s[(t * 4 + i) * 64 + lane], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2f[t][i + 1], h1s[(t * 4 + i + 1) * 64 + lane], a1, 0, 0, 0);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) h2s[(w * 4 + i) * 64 + lane] = policy_act<RELU>(a0[i] + a1[i] + b2v[i]);
    }
    __syncthreads();
    if (w == 0) {
    // ---- layer 3 (action_net, 4 outputs padded to a 16-unit tile), wave 0 ----
    f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
    for (int u = 0; u < T2; ++u)
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3f[u][i], h2s[(u * 4 + i) * 64 + lane], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3f[u][i + 1], h2s[(u * 4 + i + 1) * 64 + lane], o1, 0, 0, 0);
        }
    // lanes 0..15 hold the 4 outputs of row (lane & 15)
    if (g == 0 && live) {
    float a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float m = o0[i] + o1[i] + b3v[i];
        a[i] = m < -1.0f ? -1.0f : (m > 1.0f ? 1.0f : m);     // np.clip(actions, low, high)
    }
    float4 out;
    if (mode == POLICY_RAW) {
        out = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        // action[3] = 0; target = pose + a * [1, 1, 1, pi] (RELATIVE, pose = obs[[0,1,2,5]]) or
        // a * [1, 1, 1, pi] (ABSOLUTE); yaw = map2pi(.) -- float32 action x float64 scale
        const bool rel = mode == POLICY_RELATIVE;
        const double px = rel ? double(xrow[0]) : 0.0, py = rel ? double(xrow[1]) : 0.0,
                     pz = rel ? double(xrow[2]) : 0.0, pyaw = rel ? double(xrow[5]) : 0.0;
        out = make_float4(float(px + double(a[0])), float(py + double(a[1])), float(pz + double(a[2])),
                          float(map2pi_d(pyaw + 0.0 * 3.141592653589793)));
    }
    reinterpret_cast<float4*>(act)[r] = out;
    }
    }
    __syncthreads();          // h1s / h2s are rewritten by the next row tile
    }
}

// ---- PPO rollout step: actor + critic + diagonal-Gaussian sample ----------
// SB3 2.3.2 OnPolicyAlgorithm.collect_rollouts: actions, values, log_probs = policy(obs) with
// ActorCriticPolicy.forward(obs, deterministic=False): latent_pi / latent_vf = the two MLPs of
// mlp_extractor, mean = action_net(latent_pi), value = value_net(latent_vf),
// DiagGaussianDistribution(mean, exp(log_std)).sample() = mean + std * eps, log_prob = sum over the
// action dims of Normal.log_prob; the env then gets clip(action, low, high) (and here the
// RLController transform).  One block = 16 rows and 2 NW waves: waves [0, NW) run the actor's
// hidden layers, waves [NW, 2 NW) the critic's, on their own LDS tiles (same barrier sequence);
// wave 0 finishes the action, wave NW the value.  eps: one Philox4x32-10 block per row, counter
// {row, counter, kTagPolicy, 0}, Box-Muller by normal_pair_f (the oracle's restatement draws the
// same floats).
constexpr uint32_t kTagPolicy = 0x504f4c00u;   // "POL"

struct PolicySampleArgs {
    const float* actor;   PolicyLayout La;      // fragment blobs (build_blob) of the two MLPs
    const float* critic;  PolicyLayout Lc;
    const float* log_std;                       // [act_dim]
    const float* obs; int rows, obs_stride, mode, act_dim;
    uint64_t seed; uint32_t counter;
    float* env_act;     // [rows][act_dim == 4 ? 4 : act_dim] clip + transform
    float* action;      // [rows][act_dim] the sample (rollout-buffer action)
    float* value;       // [rows]
    float* log_prob;    // [rows]
    float* eps;         // [rows][act_dim] or null
};

// hidden layers of one MLP for the 16 rows of xb: unit tile w of layer 1 / 2 into h1s / h2s (two
// barriers, taken by every wave of the block)
template <int T1, int T2, bool RELU>
__device__ __forceinline__ void policy_hidden(const float* __restrict__ blob, const PolicyLayout& L, int w, int lane,
                                              const float (&xb)[kPolicyS1], float* h1s, float* h2s) {
    const int g = lane >> 4;
    const bool l1 = w < T1, l2 = w < T2;
    if (l1) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int s = 0; s < kPolicyS1; s += 2) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f1 + (w * kPolicyS1 + s) * 64 + lane], xb[s], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f1 + (w * kPolicyS1 + s + 1) * 64 + lane], xb[s + 1], a1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            h1s[(w * 4 + i) * 64 + lane] = policy_act<RELU>(a0[i] + a1[i] + blob[L.b1 + 16 * w + 4 * g + i]);
    }
    __syncthreads();
    if (l2) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int t = 0; t < T1; ++t)
#pragma unroll
            for (int i = 0; i < 4; i += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f2 + ((w * T1 + t) * 4 + i) * 64 + lane],
                                                          h1s[(t * 4 + i) * 64 + lane], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f2 + ((w * T1 + t) * 4 + i + 1) * 64 + lane],
                                                          h1s[(t * 4 + i + 1) * 64 + lane], a1, 0, 0, 0);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            h2s[(w * 4 + i) * 64 + lane] = policy_act<RELU>(a0[i] + a1[i] + blob[L.b2 + 16 * w + 4 * g + i]);
    }
    __syncthreads();
}

// the output layer (a 16-unit tile, outputs < n_out live) of the MLP whose layer-2 tiles are in h2s
template <int T2>
__device__ __forceinline__ f32x4 policy_out(const float* __restrict__ blob, const PolicyLayout& L, int lane,
                                            const float* h2s) {
    f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
    for (int u = 0; u < T2; ++u)
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f3 + (u * 4 + i) * 64 + lane], h2s[(u * 4 + i) * 64 + lane],
                                                      o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f3 + (u * 4 + i + 1) * 64 + lane],
                                                      h2s[(u * 4 + i + 1) * 64 + lane], o1, 0, 0, 0);
        }
    return o0 + o1;
}

template <int T1, int T2, bool RELU>
__global__ void __launch_bounds__(1024) policy_sample_kernel(PolicySampleArgs a) {
    constexpr int NW = T1 > T2 ? T1 : T2;
    __shared__ float h1s[2][T1 * 4 * 64];
    __shared__ float h2s[2][T2 * 4 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int net = wave >= NW ? 1 : 0;            // 0 actor, 1 critic
    const int w = wave - net * NW;
    const int g = lane >> 4;
    const int row0 = blockIdx.x * 16;
    const int r = row0 + (lane & 15);
    const bool live = r < a.rows;
    const float* xrow = a.obs + size_t(live ? r : row0) * a.obs_stride;
    const PolicyLayout& L = net ? a.Lc : a.La;
    const float* blob = net ? a.critic : a.actor;
    float xb[kPolicyS1];
#pragma unroll
    for (int s = 0; s < kPolicyS1; ++s) {
        const int k = 4 * s + g;
        const float v = xrow[k < L.in_dim ? k : 0];
        xb[s] = (live && k < L.in_dim) ? v : 0.0f;
    }
    policy_hidden<T1, T2, RELU>(blob, L, w, lane, xb, h1s[net], h2s[net]);
    if (w != 0) return;                              // waves 0 / NW finish (wave-uniform exit)
    const f32x4 o = policy_out<T2>(blob, L, lane, h2s[net]);   // the MFMA needs all 64 lanes
    if (g != 0 || !live) return;                     // lanes 0..15: the outputs of row lane & 15
    if (net == 1) {                                  // value_net: output 0
        a.value[r] = o[0] + blob[L.b3];
        return;
    }
    // Philox block of this row -> 4 standard normals (act_dim <= 4 of them used)
    const U4 u = philox4x32_10(U4{uint32_t(r), a.counter, kTagPolicy, 0u}, uint32_t(a.seed), uint32_t(a.seed >> 32));
    float eps[4];
    normal_pair_f(u.a, u.b, &eps[0], &eps[1]);
    normal_pair_f(u.c, u.d, &eps[2], &eps[3]);
    float act[4], clipped[4], lp = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool on = i < a.act_dim;
        const float mean = o[i] + blob[L.b3 + i];
        const float ls = on ? a.log_std[i] : 0.0f;
        const float sd = expf(ls);
        const float x = mean + sd * eps[i];
        // torch Normal.log_prob: -((x - loc)^2) / (2 var) - log(scale) - log(sqrt(2 pi))
        const float d = x - mean;
        const float l = -(d * d) / (2.0f * sd * sd) - ls - 0.91893853320467274f;
        lp += on ? l : 0.0f;
        act[i] = x;
        clipped[i] = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
        if (on) {
            a.action[size_t(r) * a.act_dim + i] = x;
            if (a.eps) a.eps[size_t(r) * a.act_dim + i] = eps[i];
        }
    }
    (void)act;
    a.log_prob[r] = lp;
    if (a.mode == POLICY_RAW) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < a.act_dim) a.env_act[size_t(r) * a.act_dim + i] = clipped[i];
    } else {   // RLController / RLControllerTwoGates transform of the clipped action (act_dim 4)
        const bool rel = a.mode == POLICY_RELATIVE;
        const double px = rel ? double(xrow[0]) : 0.0, py = rel ? double(xrow[1]) : 0.0,
                     pz = rel ? double(xrow[2]) : 0.0, pyaw = rel ? double(xrow[5]) : 0.0;
        reinterpret_cast<float4*>(a.env_act)[r] =
            make_float4(float(px + double(clipped[0])), float(py + double(clipped[1])), float(pz + double(clipped[2])),
                        float(map2pi_d(pyaw + 0.0 * 3.141592653589793)));
    }
}

// ---- wide path: in_dim <= kPolicyMaxIn, act_dim <= kPolicyMaxOut ---------------------------------
// HoverAviary(act=RPM) rows are 72 floats; SB3's MlpPolicy sees MultiHoverAviary as one joint agent
// per env (N D inputs, N A outputs: 144 -> 8 for two RPM drones, 576 -> 32 for eight).  The narrow
// kernels above keep every policy with in_dim <= 64 and act_dim <= 4; these serve the rest (and any
// policy under ADRP_POLICY_WIDE=1).  One block = 16 rows, as above.
//
// Obs tile.  Layer 1 has S1 = ceil(in_dim / 4) k-steps, taken kPolicyChunk = 16 at a time (64 obs
// columns, L.s1 / 16 chunks: a block-uniform runtime loop, in_dim is no template parameter).  The
// whole block stages one chunk of its 16 rows into LDS in k-major order, xs[k][16], so that lane
// (row = lane & 15, g = lane >> 4) reads the B operand of k-step s at xs[(4 s + g) 16 + row] =
// xs[64 s + lane]: consecutive, conflict-free.  Rows whose stride and base are 16-byte aligned are
// read as float4 (16 rows x 16 column quads per pass), others float by float (16 rows x 4 columns
// per wave load, LDS index = element index); columns >= in_dim and rows >= rows are staged as
// zeros.  Two 4 KiB buffers: chunk c + 1's global loads (obs into registers, and the wave's 16
// weight fragments of that chunk from the L2-resident blob) are issued before chunk c's MFMAs and
// land in LDS / the current-fragment registers after them; one barrier per chunk.  LDS: 8 KiB of
// obs + h1s + h2s per net, <= 40 KiB for the 128/128 actor + critic (the whole 36 KiB tile beside
// them would pass 64 KiB).
//
// Accumulation order (the f32-input MFMA is bitwise an fmaf chain, so this defines the result):
// two chains per wave over all chunks, even k-steps s = 0, 2, 4, .. on a0 and odd ones on a1, each
// ascending in s across the chunk boundaries; then a0 + a1 + b1.  That is the narrow kernel's
// order, so for in_dim <= 64 (one chunk) the wide path gives the narrow path's bits.  Layers 2 and
// 3: as the narrow kernels (k-steps (t, i) even i on chain 0, odd on chain 1, o0 + o1 + b).
//
// Output layer.  T3 = L.t3 tiles of 16 outputs; lane (row, g) of tile u holds outputs 16 u + 4 g + i
// (i = accumulator register), all four lane groups live; tile u is computed by wave u % NW.  RAW
// stores [rows][act_dim] contiguous, bounded by act_dim; RELATIVE / ABSOLUTE (act_dim 4) store the
// float4 setpoint from lanes g == 0 of tile 0.
//
// Sampling.  One Philox4x32-10 block per (row, output quad q = 4 u + g), counter {row, counter,
// kTagPolicy, q}; normal_pair_f of its word pairs (a, b), (c, d) gives the standard normals of outputs
// 4 q .. 4 q + 3.  Quad 0 is the narrow kernel's stream.  log_prob: each lane sums its four terms
// in ascending output index (outputs >= act_dim add 0) into lps[q][row] (LDS); after a barrier lane
// (row, 0) of wave 0 adds the quads in ascending q, starting from quad 0's sum.  With act_dim <= 4
// that is the narrow kernel's sum.
template <int NT>
struct PolicyStage {
    static constexpr int V4 = (256 + NT - 1) / NT;      // float4 (or 4 floats) per thread per chunk
    float4 v[V4];
};

// chunk c of rows row0 .. row0 + 15 -> registers (zeros outside rows x in_dim)
template <int NT>
__device__ __forceinline__ void policy_stage_load(PolicyStage<NT>& st, const float* __restrict__ obs, int rows, int stride,
                                                  int in_dim, int row0, int c, bool vec, int tid) {
#pragma unroll
    for (int v = 0; v < PolicyStage<NT>::V4; ++v) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec) {
            const int e = tid + v * NT;                  // 16 rows x 16 column quads
            const int r = row0 + (e & 15), col = 64 * c + 4 * (e >> 4);
            if (e < 256 && r < rows && col < in_dim) {   // stride % 4 == 0 and col < in_dim <= stride: col + 3 < stride
                x = *reinterpret_cast<const float4*>(obs + size_t(r) * stride + col);
                if (col + 1 >= in_dim) x.y = 0.f;
                if (col + 2 >= in_dim) x.z = 0.f;
                if (col + 3 >= in_dim) x.w = 0.f;
            }
        } else {
            float f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = tid + (4 * v + j) * NT;    // 16 rows x 64 columns
                const int r = row0 + (e & 15), col = 64 * c + (e >> 4);
                f[j] = (e < 1024 && r < rows && col < in_dim) ? obs[size_t(r) * stride + col] : 0.f;
            }
            x = make_float4(f[0], f[1], f[2], f[3]);
        }
        st.v[v] = x;
    }
}

// registers -> xs[k][16] (1024 floats)
template <int NT>
__device__ __forceinline__ void policy_stage_store(const PolicyStage<NT>& st, float* xs, bool vec, int tid) {
#pragma unroll
    for (int v = 0; v < PolicyStage<NT>::V4; ++v) {
        const float f[4] = {st.v[v].x, st.v[v].y, st.v[v].z, st.v[v].w};
        if (vec) {
            const int e = tid + v * NT;
            if (e < 256) {
                const int row = e & 15, k = 4 * (e >> 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) xs[(k + j) * 16 + row] = f[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = tid + (4 * v + j) * NT;    // (e >> 4) * 16 + (e & 15) == e
                if (e < 1024) xs[e] = f[j];
            }
        }
    }
}

// layer 1 of unit tile w (active waves; the others only stage): the chunk loop.  Taken by every
// wave of the block (L.s1 / 16 + 1 barriers).  xs: [2][1024] floats.
template <int NT>
__device__ __forceinline__ void policy_wide_l1(const float* __restrict__ blob, const PolicyLayout& L, bool active, int w,
                                               int lane, int tid, const float* __restrict__ obs, int rows, int stride,
                                               int row0, float* xs, f32x4& a0, f32x4& a1) {
    const int nc = L.s1 / kPolicyChunk;
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(obs) & 15) == 0;   // block-uniform
    const float* wf = blob + L.f1 + size_t(active ? w : 0) * L.s1 * 64 + lane;
    PolicyStage<NT> st;
    float wc[kPolicyChunk], wn[kPolicyChunk];
    policy_stage_load<NT>(st, obs, rows, stride, L.in_dim, row0, 0, vec, tid);
#pragma unroll
    for (int s = 0; s < kPolicyChunk; ++s) wc[s] = active ? wf[s * 64] : 0.f;
    policy_stage_store<NT>(st, xs, vec, tid);
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
        const bool more = c + 1 < nc;
        if (more) {                                      // chunk c + 1: loads in flight over chunk c's MFMAs
            policy_stage_load<NT>(st, obs, rows, stride, L.in_dim, row0, c + 1, vec, tid);
            if (active) {
#pragma unroll
                for (int s = 0; s < kPolicyChunk; ++s) wn[s] = wf[((c + 1) * kPolicyChunk + s) * 64];
            }
        }
        if (active) {
            const float* x = xs + (c & 1) * 1024 + lane;
#pragma unroll
            for (int s = 0; s < kPolicyChunk; s += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[s], x[s * 64], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[s + 1], x[(s + 1) * 64], a1, 0, 0, 0);
            }
        }
        if (more) {
            policy_stage_store<NT>(st, xs + ((c + 1) & 1) * 1024, vec, tid);
            if (active) {
#pragma unroll
                for (int s = 0; s < kPolicyChunk; ++s) wc[s] = wn[s];
            }
        }
        __syncthreads();    // chunk c + 1 staged; chunk c's buffer free for chunk c + 2
    }
}

// activation of layer 1's accumulators into h1s, layer 2 of unit tile w into h2s (policy_hidden's
// second half; two barriers, taken by every wave)
template <int T1, int T2, bool RELU>
__device__ __forceinline__ void policy_wide_l2(const float* __restrict__ blob, const PolicyLayout& L, int w, int lane,
                                               const f32x4& c0, const f32x4& c1, float* h1s, float* h2s) {
    const int g = lane >> 4;
    if (w < T1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            h1s[(w * 4 + i) * 64 + lane] = policy_act<RELU>(c0[i] + c1[i] + blob[L.b1 + 16 * w + 4 * g + i]);
    }
    __syncthreads();
    if (w < T2) {
        f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int t = 0; t < T1; ++t)
#pragma unroll
            for (int i = 0; i < 4; i += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f2 + ((w * T1 + t) * 4 + i) * 64 + lane],
                                                          h1s[(t * 4 + i) * 64 + lane], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(blob[L.f2 + ((w * T1 + t) * 4 + i + 1) * 64 + lane],
                                                          h1s[(t * 4 + i + 1) * 64 + lane], a1, 0, 0, 0);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            h2s[(w * 4 + i) * 64 + lane] = policy_act<RELU>(a0[i] + a1[i] + blob[L.b2 + 16 * w + 4 * g + i]);
    }
    __syncthreads();
}

// output tile u3 (outputs 16 u3 .. 16 u3 + 15) of the MLP whose layer-2 tiles are in h2s, without the bias
template <int T2>
__device__ __forceinline__ f32x4 policy_out_tile(const float* __restrict__ blob, const PolicyLayout& L, int u3, int lane,
                                                 const float* h2s) {
    f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = o0;
    const float* f = blob + L.f3 + u3 * T2 * 4 * 64 + lane;
#pragma unroll
    for (int u = 0; u < T2; ++u)
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[(u * 4 + i) * 64], h2s[(u * 4 + i) * 64 + lane], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f[(u * 4 + i + 1) * 64], h2s[(u * 4 + i + 1) * 64 + lane], o1, 0, 0, 0);
        }
    return o0 + o1;
}

// RLController / RLControllerTwoGates transform of a clipped 4-action (mode != RAW)
__device__ __forceinline__ float4 policy_setpoint(const float (&a)[4], const float* xrow, int mode) {
    const bool rel = mode == POLICY_RELATIVE;
    const double px = rel ? double(xrow[0]) : 0.0, py = rel ? double(xrow[1]) : 0.0, pz = rel ? double(xrow[2]) : 0.0,
                 pyaw = rel ? double(xrow[5]) : 0.0;
    return make_float4(float(px + double(a[0])), float(py + double(a[1])), float(pz + double(a[2])),
                       float(map2pi_d(pyaw + 0.0 * 3.141592653589793)));
}

template <int T1, int T2, bool RELU>
__global__ void __launch_bounds__(512) policy_wide_kernel(const float* __restrict__ blob, PolicyLayout L,
                                                          const float* __restrict__ obs, int rows, int obs_stride,
                                                          float* __restrict__ act, int mode) {
    constexpr int NW = T1 > T2 ? T1 : T2;
    __shared__ float xs[2 * 1024];
    __shared__ float h1s[T1 * 4 * 64];
    __shared__ float h2s[T2 * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int row0 = blockIdx.x * 16;
    const int r = row0 + (lane & 15);
    const bool live = r < rows;
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
    policy_wide_l1<64 * NW>(blob, L, w < T1, w, lane, tid, obs, rows, obs_stride, row0, xs, a0, a1);
    policy_wide_l2<T1, T2, RELU>(blob, L, w, lane, a0, a1, h1s, h2s);
    for (int u3 = w; u3 < L.t3; u3 += NW) {              // wave-uniform
        const f32x4 o = policy_out_tile<T2>(blob, L, u3, lane, h2s);   // the MFMA needs all 64 lanes
        float a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float m = o[i] + blob[L.b3 + 16 * u3 + 4 * g + i];
            a[i] = m < -1.0f ? -1.0f : (m > 1.0f ? 1.0f : m);         // np.clip(actions, low, high)
        }
        if (mode == POLICY_RAW) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 16 * u3 + 4 * g + i;
                if (live && j < L.n_out) act[size_t(r) * L.n_out + j] = a[i];
            }
        } else if (live && u3 == 0 && g == 0) {
            reinterpret_cast<float4*>(act)[r] = policy_setpoint(a, obs + size_t(r) * obs_stride, mode);
        }
    }
}

template <int T1, int T2, bool RELU>
__global__ void __launch_bounds__(1024) policy_sample_wide_kernel(PolicySampleArgs a) {
    constexpr int NW = T1 > T2 ? T1 : T2;
    __shared__ float xs[2 * 1024];
    __shared__ float h1s[2][T1 * 4 * 64];
    __shared__ float h2s[2][T2 * 4 * 64];
    __shared__ float lps[(kPolicyMaxOut / 4) * 16];      // [quad][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int net = wave >= NW ? 1 : 0;                  // 0 actor, 1 critic
    const int w = wave - net * NW;
    const int row0 = blockIdx.x * 16;
    const int r = row0 + (lane & 15);
    const bool live = r < a.rows;
    const PolicyLayout& L = net ? a.Lc : a.La;
    const float* blob = net ? a.critic : a.actor;
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0;
    // one staged tile for both nets (La.s1 == Lc.s1, La.in_dim == Lc.in_dim)
    policy_wide_l1<128 * NW>(blob, L, w < T1, w, lane, tid, a.obs, a.rows, a.obs_stride, row0, xs, c0, c1);
    policy_wide_l2<T1, T2, RELU>(blob, L, w, lane, c0, c1, h1s[net], h2s[net]);
    if (net == 1) {
        if (w == 0) {                                    // value_net: output 0
            const f32x4 o = policy_out_tile<T2>(blob, L, 0, lane, h2s[1]);
            if (g == 0 && live) a.value[r] = o[0] + blob[L.b3];
        }
    } else {
        for (int u3 = w; u3 < L.t3; u3 += NW) {          // wave-uniform
            const f32x4 o = policy_out_tile<T2>(blob, L, u3, lane, h2s[0]);
            const int q = 4 * u3 + g;
            const U4 u = philox4x32_10(U4{uint32_t(r), a.counter, kTagPolicy, uint32_t(q)}, uint32_t(a.seed),
                                       uint32_t(a.seed >> 32));
            float eps[4];
            normal_pair_f(u.a, u.b, &eps[0], &eps[1]);
            normal_pair_f(u.c, u.d, &eps[2], &eps[3]);
            float clipped[4], lp = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * q + i;
                const bool on = j < a.act_dim;
                const float mean = o[i] + blob[L.b3 + j];
                const float ls = on ? a.log_std[j] : 0.0f;
                const float sd = expf(ls);
                const float x = mean + sd * eps[i];
                // torch Normal.log_prob: -((x - loc)^2) / (2 var) - log(scale) - log(sqrt(2 pi))
                const float d = x - mean;
                const float l = -(d * d) / (2.0f * sd * sd) - ls - 0.91893853320467274f;
                lp += on ? l : 0.0f;
                clipped[i] = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
                if (on && live) {
                    a.action[size_t(r) * a.act_dim + j] = x;
                    if (a.eps) a.eps[size_t(r) * a.act_dim + j] = eps[i];
                    if (a.mode == POLICY_RAW) a.env_act[size_t(r) * a.act_dim + j] = clipped[i];
                }
            }
            lps[q * 16 + (lane & 15)] = lp;
            if (a.mode != POLICY_RAW && q == 0 && live)  // act_dim 4: the transform of the clipped action
                reinterpret_cast<float4*>(a.env_act)[r] = policy_setpoint(clipped, a.obs + size_t(r) * a.obs_stride, a.mode);
        }
    }
    __syncthreads();                                     // every quad's sum is in lps
    if (wave == 0 && g == 0 && live) {
        float lp = lps[lane & 15];
        for (int q = 1; q < 4 * a.La.t3; ++q) lp += lps[q * 16 + (lane & 15)];
        a.log_prob[r] = lp;
    }
}

// host launchers (policy_wide.hip): the T1 x T2 x RELU instantiations live in their own translation unit
hipError_t policy_wide_launch(const float* blob, const PolicyLayout& L, int h1, int h2, int relu, const float* obs, int rows,
                              int obs_stride, float* act, int mode, hipStream_t s);
hipError_t policy_sample_wide_launch(int h1, int h2, int relu, const PolicySampleArgs& a, hipStream_t s);

}  // namespace adrp
