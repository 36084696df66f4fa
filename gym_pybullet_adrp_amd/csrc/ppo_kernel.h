// ppo_kernel.h — on-device PPO minibatch update for the MlpPolicy DevicePolicy serves: the clipped
// surrogate loss of stable_baselines3 2.3.2 PPO.train() (restated from its published code: SB3 is
// not pinned here), its gradient with respect to the 13 parameter tensors, clip_grad_norm_, Adam and
// the re-pack of the updated parameters into the policy's MFMA fragment blobs.
//
// Four launches per minibatch, each grid-wide dependency a kernel boundary:
//   ppo_advstat_kernel   64 partial sums of the minibatch's advantages and their squares
//   ppo_grad_kernel      forward, loss, backward; one partial gradient slab per block
//   ppo_reduce_kernel    raw gradient = sum of the slabs in ascending block order; squared-norm
//                        partials; the five statistics; Adam's step count t += 1
//   ppo_adam_kernel      total norm (fixed order), clip, Adam, master parameters -> fragment blobs
// No atomics, no block waits on another: the same inputs give the same bits.
//
// The target_kl stop is a latch in the learner's device memory, int stop[4] (adrp_ppo_train_begin clears it):
//   stop[0]  1 once a minibatch's approx_kl exceeded 1.5 target_kl (written by ppo_reduce_kernel block 0)
//   stop[1]  optimizer steps applied since the clear (the same thread)
//   stop[2]  stop[0] as the Adam launch of the tripping minibatch saw it (its block 0 writes it)
// Every kernel returns at entry when the latch is set: ppo_advstat_kernel, ppo_grad_kernel and
// ppo_adam_kernel read stop[0], ppo_reduce_kernel reads stop[2], since its own block 0 is the writer of
// stop[0].  So every read is of a word that an earlier launch wrote, never the same launch, and the kernel
// boundary orders it: the Adam launch of the tripping minibatch skips its step, every later launch is a no-op.
//
// ppo_grad_kernel.  One block = 2 NW waves as policy_sample_wide_kernel (waves [0, NW) the actor,
// [NW, 2 NW) the critic, wave w owns hidden-unit tile w), working through groups of RG 16-row tiles
// (group g, g + gridDim.x, ..).  Rows are gathered by idx from the rollout buffers.  All products
// are v_mfma_f32_16x16x4_f32.  Forward, as the policy kernels (accumulator tile [unit = 4 g + reg]
// [row = lane & 15], handed on through LDS as the next B operand):
//   Z1ᵀ = W1 Xᵀ, Z2ᵀ = W2 A1ᵀ, Oᵀ = W3 A2ᵀ
// Backward activations, the same hand-off with the transposed fragment images w3t / w2t (k runs over
// the output index): dA2ᵀ = W3ᵀ dOᵀ, dA1ᵀ = W2ᵀ dZ2ᵀ, dZ = dA act'(A).
// Weight gradients, k over the 16 rows of a tile (4 k-steps), both operands read transposed from
// the LDS tiles: dW3 += dOᵀ A2, dW2 += dZ2ᵀ A1 in registers over all of the block's row tiles;
// dW1 = dZ1ᵀ X once per group, from the group's dZ1 tiles kept in LDS and X re-read from the
// buffer (L2), one 16 x 16 tile of dW1 at a time, so that in_dim costs no registers.  A block's
// first group starts its dW1 tiles at zero; a later group adds to the block's own slab.
// Summation order: within a block ascending row tile (k-step s = 0..3 inside a tile), bias and
// log_std gradients per lane over the row tiles and then a xor-butterfly over the 16 row lanes;
// across blocks four interleaved ascending chains (ppo_reduce_kernel).  The advantage mean / std come
// from 64 double partial sums added in a fixed butterfly by every wave that needs them.
#pragma once

#include "policy_kernel.h"

namespace adrp {

constexpr int kPpoAdvBlocks = 64;     // partial sums of the advantage statistics (one per lane of a wave)
constexpr int kPpoTensors = 13;        // policy.ACTOR_KEYS + policy.CRITIC_KEYS, in that order

// where everything lives (device pointers); off[k] = start of tensor k in the flat parameter
// vector (torch layout), off[13] = its length
struct PpoDesc {
    int off[kPpoTensors + 1];
    int in_dim, h1, h2, act_dim;
    PolicyLayout L[2];                 // actor, critic blob layouts (build_blob)
    float* blob[2];
    float* log_std;
    float* w2t[2];                     // fragment (t, u, i), lane l: W2[16 u + 4 (l >> 4) + i][16 t + (l & 15)]
    float* w3t[2];                     // fragment (u, u3, i), lane l: W3[16 u3 + 4 (l >> 4) + i][16 u + (l & 15)]
};

// One master parameter <-> its places in the device images.  unpack: read the blob into *val
// (adrp_ppo_create takes the policy's weights from its blobs); otherwise write *val to the blob.
// Either way the transposed images of W2 / W3 get the value.
__device__ __forceinline__ void ppo_sync_param(const PpoDesc& d, int p, float* val, bool unpack) {
    int ti = kPpoTensors - 1;
    while (ti > 0 && p < d.off[ti]) --ti;
    const int loc = p - d.off[ti];
    if (ti == kPpoTensors - 1) {
        if (unpack) *val = d.log_std[loc]; else d.log_std[loc] = *val;
        return;
    }
    const int net = ti >= 6 ? 1 : 0, kind = ti - 6 * net;
    const PolicyLayout& L = d.L[net];
    float* blob = d.blob[net];
    const int T1 = d.h1 / 16, T2 = d.h2 / 16;
    int pos;
    if (kind == 0) {
        const int out = loc / d.in_dim, k = loc - out * d.in_dim;
        pos = L.f1 + ((out >> 4) * L.s1 + (k >> 2)) * 64 + (k & 3) * 16 + (out & 15);
    } else if (kind == 1) pos = L.b1 + loc;
    else if (kind == 2) {
        const int out = loc / d.h1, k = loc - out * d.h1;
        pos = L.f2 + (((out >> 4) * T1 + (k >> 4)) * 4 + (k & 3)) * 64 + ((k >> 2) & 3) * 16 + (out & 15);
    } else if (kind == 3) pos = L.b2 + loc;
    else if (kind == 4) {
        const int out = loc / d.h2, k = loc - out * d.h2;
        pos = L.f3 + (((out >> 4) * T2 + (k >> 4)) * 4 + (k & 3)) * 64 + ((k >> 2) & 3) * 16 + (out & 15);
    } else pos = L.b3 + loc;
    if (unpack) *val = blob[pos]; else blob[pos] = *val;
    if (kind == 2) {
        const int out = loc / d.h1, k = loc - out * d.h1;
        d.w2t[net][(((k >> 4) * T2 + (out >> 4)) * 4 + (out & 3)) * 64 + ((out >> 2) & 3) * 16 + (k & 15)] = *val;
    } else if (kind == 4) {
        const int out = loc / d.h2, k = loc - out * d.h2;
        d.w3t[net][(((k >> 4) * L.t3 + (out >> 4)) * 4 + (out & 3)) * 64 + ((out >> 2) & 3) * 16 + (k & 15)] = *val;
    }
}

#ifdef ADRP_PPO_SMALL_KERNELS   // the non-template kernels are defined once, in ppo.hip
__global__ void __launch_bounds__(256) ppo_pack_kernel(PpoDesc d, float* __restrict__ params, int unpack) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= d.off[kPpoTensors]) return;
    float v = unpack ? 0.0f : params[p];
    ppo_sync_param(d, p, &v, unpack != 0);
    if (unpack) params[p] = v;
}

// sum of one double per thread over a 256-thread block, fixed tree; the result in every thread
__device__ __forceinline__ double ppo_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// advantage statistics, stage 1: block b sums adv[idx[i]] and its square (double) over its slice
// i in [b c, (b + 1) c), c = ceil(n / kPpoAdvBlocks); thread t takes i = b c + t, + 256, .. and the
// block a fixed tree.  ppo_grad_kernel adds the kPpoAdvBlocks partials (a fixed butterfly).
__global__ void __launch_bounds__(256) ppo_advstat_kernel(const float* __restrict__ adv, const int64_t* __restrict__ idx, int n,
                                                          double* __restrict__ advpart, const int* __restrict__ stop) {
    __shared__ double red[256];
    if (stop[0] != 0) return;                            // the target_kl latch (uniform)
    const int c = (n + kPpoAdvBlocks - 1) / kPpoAdvBlocks;
    const int lo = blockIdx.x * c, hi = lo + c < n ? lo + c : n;
    double s = 0.0, q = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const double x = double(adv[idx[i]]);
        s += x;
        q += x * x;
    }
    s = ppo_block_sum(s, red);
    q = ppo_block_sum(q, red);
    if (threadIdx.x == 0) {
        advpart[2 * blockIdx.x] = s;
        advpart[2 * blockIdx.x + 1] = q;
    }
}

#endif

struct PpoGradArgs {
    PpoDesc d;
    const float* obs; int obs_stride;
    const float* actions;              // [rows][act_dim], the stored (unclipped) samples
    const float* old_values; const float* old_log_prob; const float* adv; const float* ret;
    const int64_t* idx; int n;
    const double* advpart;             // [kPpoAdvBlocks][2] sum, sum of squares (ppo_advstat_kernel); null: no normalisation
    float clip, clip_vf, vf_coef;      // clip_vf < 0: no value clipping
    float* partial;                    // [gridDim.x][off[13]]
    float* spart;                      // [gridDim.x][4]: sums of the policy term, value term, kl term, clipped rows
    int ngroups, rg;                   // groups of rg <= ppo_group_tiles<T1>() row tiles
    const int* stop;                   // the target_kl latch: stop[0] != 0, the launch does nothing
};

// the 16 x 16 LDS tile t[(reg) 64 + 16 g + row] = T[unit 4 g + reg][row] read as an MFMA operand with k
// over the rows: lane l gets T[unit l & 15][row 4 s + (l >> 4)]
__device__ __forceinline__ float ppo_lds_t(const float* tile, int s, int lane) {
    const int u = lane & 15;
    return tile[(u & 3) * 64 + (u >> 2) * 16 + 4 * s + (lane >> 4)];
}

template <bool RELU>
__device__ __forceinline__ float ppo_dact(float a) {      // act'(z) from a = act(z)
    if constexpr (RELU) return a > 0.0f ? 1.0f : 0.0f;
    else return 1.0f - a * a;
}

__device__ __forceinline__ float ppo_row_sum(float v) {   // over the 16 row lanes of a lane group, in every lane
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

template <int T1>
constexpr int ppo_group_tiles() { return T1 >= 8 ? 2 : (T1 == 4 ? 4 : 8); }

template <int T1, int T2, bool RELU>
__global__ void __launch_bounds__(128 * (T1 > T2 ? T1 : T2)) ppo_grad_kernel(PpoGradArgs a) {
    constexpr int NW = T1 > T2 ? T1 : T2;
    constexpr int NT = 128 * NW;
    constexpr int RG = ppo_group_tiles<T1>();
    constexpr int H1 = 16 * T1, H2 = 16 * T2;
    __shared__ float xs[1024];                           // one 64-column chunk of the obs tile, k-major
    __shared__ float h1s[2][T1 * 256];
    __shared__ float h2s[2][T2 * 256];
    __shared__ float dz2s[2][T2 * 256];
    __shared__ float dos[2][2 * 256];
    __shared__ float dz1s[2][RG][T1 * 256];
    __shared__ float lps[(kPolicyMaxOut / 4) * 16];      // [quad][row]
    __shared__ float vals[16], rowc[16], vcoef[16];
    __shared__ long long idxs[RG * 16];                  // the group's buffer rows
    if (a.stop[0] != 0) return;                          // the target_kl latch (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, row = lane & 15;
    const int net = wave >= NW ? 1 : 0;                  // 0 actor, 1 critic
    const int w = wave - net * NW;
    const PolicyLayout& L = a.d.L[net];
    const float* blob = a.d.blob[net];
    const float* w2t = a.d.w2t[net];
    const float* w3t = a.d.w3t[net];
    const int* off = a.d.off + 6 * net;                  // W1, b1, W2, b2, W3, b3 of this net
    const int in_dim = a.d.in_dim, act_dim = a.d.act_dim, n = a.n, stride = a.obs_stride;
    float* slab = a.partial + size_t(blockIdx.x) * a.d.off[kPpoTensors];
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(a.obs) & 15) == 0;   // block-uniform
    const int nc = L.s1 / kPolicyChunk;
    // mean and 1 / (std + 1e-8) of the minibatch's advantages (std unbiased, as torch's): every wave adds
    // the 64 partials in the same butterfly order
    float amean = 0.0f, arstd = 1.0f;
    if (a.advpart) {
        double s = a.advpart[2 * lane], q = a.advpart[2 * lane + 1];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            s += __shfl_xor(s, m);
            q += __shfl_xor(q, m);
        }
        const double mean = s / n;
        double var = (q - s * mean) / (n - 1);
        var = var > 0.0 ? var : 0.0;
        amean = float(mean);
        arstd = float(1.0 / (sqrt(var) + 1e-8));
    }
    const float invn = 1.0f / float(n);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 acc2[T1], acc3[2] = {zero, zero}, db1 = zero, db2 = zero, db3[2] = {zero, zero}, dls[2] = {zero, zero};
#pragma unroll
    for (int t = 0; t < T1; ++t) acc2[t] = zero;
    float st_pl = 0.f, st_vl = 0.f, st_kl = 0.f, st_cf = 0.f;

    // The weight fragments a wave multiplies with in every row tile, requested once, ahead of the first
    // barrier (a load issued behind a barrier costs one memory latency per stage and row tile).  With
    // 128 hidden units (16 waves, 128 VGPRs each) they stay in memory and are read where they are used.
    constexpr bool HOIST = NW < 8;
    constexpr int HT1 = HOIST ? T1 : 1, HT2 = HOIST ? T2 : 1;
    float w2r[HT1][4], w2tr[HT2][4], w3r[HT2][4], w3tr[2][4], b1r[4], b2r[4];
    if constexpr (HOIST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b1r[i] = blob[L.b1 + 16 * (w < T1 ? w : 0) + 4 * g + i];
            b2r[i] = blob[L.b2 + 16 * (w < T2 ? w : 0) + 4 * g + i];
#pragma unroll
            for (int t = 0; t < T1; ++t) w2r[t][i] = blob[L.f2 + (((w < T2 ? w : 0) * T1 + t) * 4 + i) * 64 + lane];
#pragma unroll
            for (int u = 0; u < T2; ++u) {
                w2tr[u][i] = w2t[(((w < T1 ? w : 0) * T2 + u) * 4 + i) * 64 + lane];
                w3r[u][i] = blob[L.f3 + (((w < L.t3 ? w : 0) * T2 + u) * 4 + i) * 64 + lane];     // output tile w (slot 0)
            }
#pragma unroll
            for (int u3 = 0; u3 < 2; ++u3) w3tr[u3][i] = w3t[(((w < T2 ? w : 0) * L.t3 + (u3 < L.t3 ? u3 : 0)) * 4 + i) * 64 + lane];
        }
    }
    auto W2 = [&](int t, int i) { if constexpr (HOIST) return w2r[t][i]; else return blob[L.f2 + ((w * T1 + t) * 4 + i) * 64 + lane]; };
    auto W2T = [&](int u, int i) { if constexpr (HOIST) return w2tr[u][i]; else return w2t[((w * T2 + u) * 4 + i) * 64 + lane]; };
    auto W3T = [&](int u3, int i) { if constexpr (HOIST) return w3tr[u3][i]; else return w3t[((w * L.t3 + u3) * 4 + i) * 64 + lane]; };
    auto B1 = [&](int i) { if constexpr (HOIST) return b1r[i]; else return blob[L.b1 + 16 * w + 4 * g + i]; };
    auto B2 = [&](int i) { if constexpr (HOIST) return b2r[i]; else return blob[L.b2 + 16 * w + 4 * g + i]; };

    bool first = true;
    for (int grp = blockIdx.x; grp < a.ngroups; grp += gridDim.x, first = false) {
        const int tile0 = grp * a.rg;
        for (int t = tid; t < a.rg * 16; t += NT) {      // rows beyond n: a valid row, masked everywhere below
            const int rr = tile0 * 16 + t;
            idxs[t] = a.idx[rr < n ? rr : tile0 * 16];
        }
        __syncthreads();
        int cnt = 0;
        for (int rt = 0; rt < a.rg; ++rt) {
            const int row0 = (tile0 + rt) * 16;
            if (row0 >= n) break;                        // block-uniform
            cnt = rt + 1;
            const int r = row0 + row;
            const bool live = r < n;
            const size_t src = size_t(idxs[rt * 16 + row]);
            // the row's stored quantities, requested ahead of the barriers
            float rl_olp = 0.f, rl_adv = 0.f, rl_ov = 0.f, rl_ret = 0.f, actv[2][4];
            if (wave == 0 && g == 0) {
                rl_olp = a.old_log_prob[src]; rl_adv = a.adv[src]; rl_ov = a.old_values[src]; rl_ret = a.ret[src];
            }
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 16 * (w + k * NW) + 4 * g + i;
                    actv[k][i] = (net == 0 && j < act_dim) ? a.actions[src * act_dim + j] : 0.0f;
                }

            // ---- layer 1: chunks of 64 obs columns staged k-major, xs[k][16] (policy_wide_l1's tile) ----
            f32x4 c0 = zero, c1 = zero;
            for (int c = 0; c < nc; ++c) {
                float wc[kPolicyChunk];                  // in flight with the obs loads
                {
                    const float* wf = blob + L.f1 + (size_t(w < T1 ? w : 0) * L.s1 + c * kPolicyChunk) * 64 + lane;
#pragma unroll
                    for (int s = 0; s < kPolicyChunk; ++s) wc[s] = wf[s * 64];
                }
                if (vec) {
                    for (int e = tid; e < 256; e += NT) {          // 16 rows x 16 column quads
                        const int rr = row0 + (e & 15), col = 64 * c + 4 * (e >> 4);
                        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (rr < n && col < in_dim) {              // stride % 4 == 0 and col < in_dim <= stride
                            x = *reinterpret_cast<const float4*>(a.obs + size_t(idxs[rt * 16 + (e & 15)]) * stride + col);
                            if (col + 1 >= in_dim) x.y = 0.f;
                            if (col + 2 >= in_dim) x.z = 0.f;
                            if (col + 3 >= in_dim) x.w = 0.f;
                        }
                        const int k = 4 * (e >> 4);
                        xs[(k + 0) * 16 + (e & 15)] = x.x;
                        xs[(k + 1) * 16 + (e & 15)] = x.y;
                        xs[(k + 2) * 16 + (e & 15)] = x.z;
                        xs[(k + 3) * 16 + (e & 15)] = x.w;
                    }
                } else {
                    for (int e = tid; e < 1024; e += NT) {         // 16 rows x 64 columns
                        const int rr = row0 + (e & 15), col = 64 * c + (e >> 4);
                        xs[e] = (rr < n && col < in_dim) ? a.obs[size_t(idxs[rt * 16 + (e & 15)]) * stride + col] : 0.f;
                    }
                }
                __syncthreads();
                if (w < T1) {
#pragma unroll
                    for (int s = 0; s < kPolicyChunk; s += 2) {
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[s], xs[s * 64 + lane], c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[s + 1], xs[(s + 1) * 64 + lane], c1, 0, 0, 0);
                    }
                }
                __syncthreads();
            }
            float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
            if (w < T1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a1[i] = policy_act<RELU>(c0[i] + c1[i] + B1(i));
                    h1s[net][(w * 4 + i) * 64 + lane] = a1[i];
                }
            }
            __syncthreads();
            // ---- layer 2 ----
            if (w < T2) {
                f32x4 e0 = zero, e1 = zero;
#pragma unroll
                for (int t = 0; t < T1; ++t)
#pragma unroll
                    for (int i = 0; i < 4; i += 2) {
                        e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(W2(t, i), h1s[net][(t * 4 + i) * 64 + lane], e0, 0, 0, 0);
                        e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(W2(t, i + 1), h1s[net][(t * 4 + i + 1) * 64 + lane], e1, 0, 0, 0);
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a2[i] = policy_act<RELU>(e0[i] + e1[i] + B2(i));
                    h2s[net][(w * 4 + i) * 64 + lane] = a2[i];
                }
            }
            __syncthreads();
            // ---- output layer: tile u3 on wave u3 % NW (slot k = u3 / NW); log-prob terms of the actor ----
            float diff[2][4], iv[2][4];                  // a - mean, 1 / sigma^2 (0 beyond act_dim)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int u3 = w + k * NW;
#pragma unroll
                for (int i = 0; i < 4; ++i) diff[k][i] = iv[k][i] = 0.f;
                if (u3 >= L.t3) continue;                // wave-uniform
                f32x4 o;
                if (HOIST && k == 0) {
                    f32x4 o0 = zero, o1 = zero;
#pragma unroll
                    for (int u = 0; u < T2; ++u)
#pragma unroll
                        for (int i = 0; i < 4; i += 2) {
                            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3r[u][i], h2s[net][(u * 4 + i) * 64 + lane], o0, 0, 0, 0);
                            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3r[u][i + 1], h2s[net][(u * 4 + i + 1) * 64 + lane], o1, 0, 0, 0);
                        }
                    o = o0 + o1;
                } else {
                    o = policy_out_tile<T2>(blob, L, u3, lane, h2s[net]);
                }
                if (net == 1) {
                    if (g == 0) vals[row] = o[0] + blob[L.b3];
                    continue;
                }
                const int q = 4 * u3 + g;
                float lp = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 4 * q + i;
                    const bool on = j < act_dim;
                    const float mean = o[i] + blob[L.b3 + j];
                    const float ls = on ? a.d.log_std[j] : 0.0f;
                    const float sd = expf(ls);
                    const float x = on ? actv[k][i] : mean;
                    // torch Normal.log_prob: -((x - loc)^2) / (2 var) - log(scale) - log(sqrt(2 pi))
                    const float dd = x - mean;
                    const float l = -(dd * dd) / (2.0f * sd * sd) - ls - 0.91893853320467274f;
                    lp += on ? l : 0.0f;
                    diff[k][i] = on ? dd : 0.0f;
                    iv[k][i] = on ? 1.0f / (sd * sd) : 0.0f;
                }
                lps[q * 16 + row] = lp;
            }
            __syncthreads();
            // ---- the loss of the 16 rows: d loss / d log_prob and d loss / d value per row ----
            if (wave == 0 && g == 0) {
                float lp = lps[row];
                for (int q = 1; q < 4 * a.d.L[0].t3; ++q) lp += lps[q * 16 + row];
                const float d = lp - rl_olp;
                const float ratio = expf(d);
                const float advn = (rl_adv - amean) * arstd;
                const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
                const float s1 = advn * ratio;
                const float s2 = advn * (ratio < lo ? lo : (ratio > hi ? hi : ratio));
                const bool clipped = ratio < lo || ratio > hi;
                // torch.min sends the gradient to the smaller argument (both when equal); the clamped
                // one passes none outside [lo, hi]
                float glp = (!clipped || s1 < s2) ? -invn * s1 : 0.0f;
                const float v = vals[row], ov = rl_ov, rt_ = rl_ret;
                float vp = v;
                bool pass = true;
                if (a.clip_vf >= 0.0f) {
                    const float dv = v - ov;
                    pass = dv >= -a.clip_vf && dv <= a.clip_vf;
                    vp = ov + (dv < -a.clip_vf ? -a.clip_vf : (dv > a.clip_vf ? a.clip_vf : dv));
                }
                const float ev = vp - rt_;
                float gv = pass ? a.vf_coef * 2.0f * invn * ev : 0.0f;
                if (live) {
                    st_pl += -(s1 < s2 ? s1 : s2);
                    st_vl += ev * ev;
                    st_kl += (ratio - 1.0f) - d;
                    st_cf += fabsf(ratio - 1.0f) > a.clip ? 1.0f : 0.0f;
                } else {
                    glp = gv = 0.0f;
                }
                rowc[row] = glp;
                vcoef[row] = gv;
            }
            __syncthreads();
            // ---- dO ----
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int u3 = w + k * NW;
                if (u3 >= L.t3) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float dm;
                    if (net == 0) {
                        const float rc = rowc[row];
                        dm = rc * diff[k][i] * iv[k][i];
                        dls[k][i] += iv[k][i] != 0.0f ? rc * (diff[k][i] * diff[k][i] * iv[k][i] - 1.0f) : 0.0f;
                    } else {
                        dm = (g == 0 && i == 0) ? vcoef[row] : 0.0f;
                    }
                    dos[net][(u3 * 4 + i) * 64 + lane] = dm;
                    db3[k][i] += dm;
                }
            }
            __syncthreads();
            // ---- dA2ᵀ = W3ᵀ dOᵀ, dZ2; dW3 += dOᵀ A2 (this wave's A2 tile) ----
            if (w < T2) {
                f32x4 e0 = zero, e1 = zero;
#pragma unroll
                for (int u3 = 0; u3 < 2; ++u3) {
                    if (u3 >= L.t3) continue;
#pragma unroll
                    for (int i = 0; i < 4; i += 2) {
                        e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(W3T(u3, i), dos[net][(u3 * 4 + i) * 64 + lane], e0, 0, 0, 0);
                        e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(W3T(u3, i + 1), dos[net][(u3 * 4 + i + 1) * 64 + lane], e1, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dz = (e0[i] + e1[i]) * ppo_dact<RELU>(a2[i]);
                    dz2s[net][(w * 4 + i) * 64 + lane] = dz;
                    db2[i] += dz;
                }
#pragma unroll
                for (int k3 = 0; k3 < 2; ++k3) {
                    if (k3 >= L.t3) continue;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc3[k3] = __builtin_amdgcn_mfma_f32_16x16x4f32(ppo_lds_t(dos[net] + k3 * 256, s, lane),
                                                                        ppo_lds_t(h2s[net] + w * 256, s, lane), acc3[k3], 0, 0, 0);
                }
            }
            __syncthreads();
            // ---- dA1ᵀ = W2ᵀ dZ2ᵀ, dZ1 (kept for the group's dW1); dW2 += dZ2ᵀ A1 ----
            if (w < T1) {
                f32x4 e0 = zero, e1 = zero;
#pragma unroll
                for (int u = 0; u < T2; ++u)
#pragma unroll
                    for (int i = 0; i < 4; i += 2) {
                        e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(W2T(u, i), dz2s[net][(u * 4 + i) * 64 + lane], e0, 0, 0, 0);
                        e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(W2T(u, i + 1), dz2s[net][(u * 4 + i + 1) * 64 + lane], e1, 0, 0, 0);
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dz = (e0[i] + e1[i]) * ppo_dact<RELU>(a1[i]);
                    dz1s[net][rt][(w * 4 + i) * 64 + lane] = dz;
                    db1[i] += dz;
                }
            }
            if (w < T2) {
#pragma unroll
                for (int t = 0; t < T1; ++t)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ppo_lds_t(dz2s[net] + w * 256, s, lane),
                                                                       ppo_lds_t(h1s[net] + t * 256, s, lane), acc2[t], 0, 0, 0);
            }
            __syncthreads();          // the tiles are rewritten by the next row tile; dz1s[.][rt] is complete
        }
        // ---- dW1 of the group: tile (unit tile w, column tile c), k over the group's rows ----
        if (w < T1) {
            const int C = (in_dim + 15) / 16;
            float xv[RG][4], xn[RG][4];                  // column tile c of X, and c + 1's loads in flight over c's products
            auto loadx = [&](float (&x)[RG][4], int c) {
                const int col = 16 * c + row;
#pragma unroll
                for (int rt = 0; rt < RG; ++rt)
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int k = rt * 16 + 4 * s + g;
                        x[rt][s] = (rt < cnt && tile0 * 16 + k < n && col < in_dim) ? a.obs[size_t(idxs[k]) * stride + col] : 0.0f;
                    }
            };
            loadx(xv, 0);
            for (int c = 0; c < C; ++c) {
                const int col = 16 * c + row;
                const bool oncol = col < in_dim;
                if (c + 1 < C) loadx(xn, c + 1);
                f32x4 acc = zero;
                float* dst = slab + off[0] + size_t(16 * w + 4 * g) * in_dim + col;
                if (!first && oncol) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = dst[size_t(i) * in_dim];
                }
#pragma unroll
                for (int rt = 0; rt < RG; ++rt) {
                    if (rt >= cnt) break;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ppo_lds_t(dz1s[net][rt] + w * 256, s, lane), xv[rt][s], acc, 0, 0, 0);
                }
                if (oncol) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[size_t(i) * in_dim] = acc[i];
                }
#pragma unroll
                for (int rt = 0; rt < RG; ++rt)
#pragma unroll
                    for (int s = 0; s < 4; ++s) xv[rt][s] = xn[rt][s];
            }
        }
        __syncthreads();              // dz1s and idxs are rewritten by the next group
    }

    // ---- this block's partial slab ----
    if (w < T2) {
#pragma unroll
        for (int t = 0; t < T1; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) slab[off[2] + (16 * w + 4 * g + i) * H1 + 16 * t + row] = acc2[t][i];
#pragma unroll
        for (int k3 = 0; k3 < 2; ++k3)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int out = 16 * k3 + 4 * g + i;
                if (k3 < L.t3 && out < L.n_out) slab[off[4] + out * H2 + 16 * w + row] = acc3[k3][i];
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float s = ppo_row_sum(db2[i]);
            if (row == 0) slab[off[3] + 16 * w + 4 * g + i] = s;
        }
    }
    if (w < T1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float s = ppo_row_sum(db1[i]);
            if (row == 0) slab[off[1] + 16 * w + 4 * g + i] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int u3 = w + k * NW;
        if (u3 >= L.t3) continue;                        // wave-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int out = 16 * u3 + 4 * g + i;
            const float s = ppo_row_sum(db3[k][i]);
            const float sl = ppo_row_sum(dls[k][i]);
            if (row == 0 && out < L.n_out) {
                slab[off[5] + out] = s;
                if (net == 0) slab[a.d.off[kPpoTensors - 1] + out] = sl;
            }
        }
    }
    if (wave == 0) {
        const float p0 = ppo_row_sum(st_pl), p1 = ppo_row_sum(st_vl), p2 = ppo_row_sum(st_kl), p3 = ppo_row_sum(st_cf);
        if (lane == 0) {
            float* sp = a.spart + 4 * blockIdx.x;
            sp[0] = p0; sp[1] = p1; sp[2] = p2; sp[3] = p3;
        }
    }
}

#ifdef ADRP_PPO_SMALL_KERNELS
// raw gradient: block = 64 consecutive parameters x 4 slices of the slabs; thread (q, j) adds slabs
// b = q, q + 4, q + 8, .. of parameter j in that order, then the four slice sums are added q = 0..3
// (+ the entropy bonus' constant gradient on log_std).  Per block the squared norm of its 64
// gradients (double, fixed tree); block 0 also the statistics and t += 1.
// The thread that counts t also decides the target_kl stop, SB3's `approx_kl_div > 1.5 * target_kl` on the
// float32 statistic widened to double (kl_thr = 1.5 target_kl, a double product of the host; a NaN compares
// false).  On a trip it sets stop[0] and leaves t and stop[1] alone: the Adam launch that follows skips.
__global__ void __launch_bounds__(256) ppo_reduce_kernel(const float* __restrict__ partial, int nb, int total, int ls_off,
                                                         float ent_coef, float* __restrict__ grad,
                                                         double* __restrict__ normpart, const float* __restrict__ spart,
                                                         int n, const float* __restrict__ log_std, int act_dim,
                                                         float* __restrict__ stats, int* __restrict__ t_dev,
                                                         int* __restrict__ stop, int kl_on, double kl_thr) {
    __shared__ double red[256];
    __shared__ float part[256];
    if (stop[2] != 0) return;                            // the latch as an earlier minibatch's Adam launch left it (uniform)
    const int q = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int p = blockIdx.x * 64 + j;
    float s = 0.0f;
    if (p < total) {
#pragma unroll 8
        for (int b = q; b < nb; b += 4) s += partial[size_t(b) * total + p];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    double sq = 0.0;
    if (q == 0 && p < total) {
        s = ((part[j] + part[64 + j]) + part[128 + j]) + part[192 + j];
        if (p >= ls_off) s -= ent_coef;                  // d (ent_coef * -mean(entropy)) / d log_std
        grad[p] = s;
        sq = double(s) * double(s);
    }
    sq = ppo_block_sum(sq, red);
    if (threadIdx.x == 0) normpart[blockIdx.x] = sq;
    if (blockIdx.x == 0) {
        const int k = threadIdx.x;
        if (k < 4) {                                     // policy term, value term, kl term, clipped rows
            double acc = 0.0;
            for (int b = 0; b < nb; ++b) acc += double(spart[4 * b + k]);
            stats[k == 0 ? 0 : (k == 1 ? 1 : k + 1)] = float(acc / n);
        } else if (k == 4) {                             // entropy_loss = -mean(entropy), the same for every row
            double e = 0.0;
            for (int jj = 0; jj < act_dim; ++jj) e += 1.4189385332046727 + double(log_std[jj]);
            stats[2] = float(-e);
        } else if (k == 5) {
            bool trip = false;
            if (kl_on) {                                 // the value lane k = 2 stores as stats[3], summed again
                double acc = 0.0;
                for (int b = 0; b < nb; ++b) acc += double(spart[4 * b + 2]);
                trip = double(float(acc / n)) > kl_thr;
            }
            if (trip) {
                stop[0] = 1;
            } else {
                t_dev[0] += 1;
                stop[1] += 1;
            }
        }
    }
}

// clip_grad_norm_ + torch.optim.Adam + re-pack, one thread per parameter; every block sums the
// norm partials in the same fixed order
__global__ void __launch_bounds__(256) ppo_adam_kernel(PpoDesc d, const float* __restrict__ grad,
                                                       const double* __restrict__ normpart, int nparts,
                                                       float* __restrict__ params, float* __restrict__ m, float* __restrict__ v,
                                                       const int* __restrict__ t_dev, double lr, double max_norm,
                                                       int* __restrict__ stop) {
    __shared__ double red[256];
    if (stop[0] != 0) {                                  // the target_kl latch (uniform): no step
        if (blockIdx.x == 0 && threadIdx.x == 0) stop[2] = 1;
        return;
    }
    double q = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) q += normpart[i];
    const double norm = sqrt(ppo_block_sum(q, red));
    const double coef = max_norm / (norm + 1e-6);
    const double scale = coef < 1.0 ? coef : 1.0;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= d.off[kPpoTensors]) return;
    const double b1 = 0.9, b2 = 0.999, eps = 1e-5;
    const double t = double(t_dev[0]);
    const double gr = double(grad[p]) * scale;
    const double mn = b1 * double(m[p]) + (1.0 - b1) * gr;
    const double vn = b2 * double(v[p]) + (1.0 - b2) * gr * gr;
    const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
    const double pn = double(params[p]) - (lr / bc1) * mn / (sqrt(vn) / sqrt(bc2) + eps);
    m[p] = float(mn);
    v[p] = float(vn);
    float pf = float(pn);
    params[p] = pf;
    ppo_sync_param(d, p, &pf, false);
}

#endif

// ppo_grad_kernel launchers (ppo_tanh.hip / ppo_relu.hip)
hipError_t ppo_grad_launch_tanh(int h1, int h2, const PpoGradArgs& a, int grid, hipStream_t s);
hipError_t ppo_grad_launch_relu(int h1, int h2, const PpoGradArgs& a, int grid, hipStream_t s);

}  // namespace adrp
