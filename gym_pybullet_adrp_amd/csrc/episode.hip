// episode.hip — on-device episode statistics (include/adrp.h: adrp_episode_step / adrp_episode_summary).
//
// Replaces, for the GPU batch, the per-step host loops that keep episode accounts in the reference's
// training script (examples/learn.py:82-94, 142): stable_baselines3 2.3.2 evaluate_policy's
// `for i in range(n_envs)` loop (current_rewards / current_lengths, episode_counts against
// episode_count_targets, the episode_rewards / episode_lengths lists) and the Monitor window
// (ep_info_buffer = deque(maxlen=stats_window_size)) behind rollout/ep_rew_mean / ep_len_mean.
// Handle-less: the caller owns every buffer (adrp_episode_io), every pointer is fixed per step, so a
// step can be captured in a HIP graph.  No atomics: one workgroup ranks the step's finishers with wave
// ballots (compact_rows_kernel's scheme), so equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/adrp.h"
#include "device_guard.h"

int seterr(adrp_t* h, int code, const std::string& msg);

namespace {

constexpr int kLanes = 1024, kWaves = kLanes / 64;

// One launch per env.step.  Pass 1 counts the step's logged finishers k (a ring needs k before the first
// write: only ranks >= k - C are stored, one writer per slot).  Pass 2 walks the envs in 1024-env chunks:
// running sums, the finisher's rank among the logged finishers (ascending env index), its log slot.
__global__ void __launch_bounds__(kLanes) episode_step_kernel(adrp_episode_io io, const float* __restrict__ rew,
                                                              const uint8_t* __restrict__ term,
                                                              const uint8_t* __restrict__ trunc) {
    __shared__ int wsum[kWaves];
    __shared__ long long wrem[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = io.num_envs, C = io.capacity;
    const int32_t* __restrict__ quota = io.quota;
    const long long total = io.meta[0];      // read by every lane before lane 0 rewrites it (barriers below)

    int mine = 0;
    for (int i = tid; i < E; i += kLanes) {
        const bool done = (term[i] | trunc[i]) != 0;
        mine += (done && (!quota || io.count[i] < quota[i])) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_down(mine, s);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    int k = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) k += wsum[w];
    __syncthreads();   // wsum is rewritten by the first chunk
    const int first = (io.ring && k > C) ? k - C : 0;   // ring: ranks below it would be overwritten within this step

    int base = 0;
    long long rem = 0;
    for (int c0 = 0; c0 < E; c0 += kLanes) {
        const int i = c0 + tid;
        bool f = false;
        double ret = 0.0;
        int len = 0, cnt = 0, q = 0;
        if (i < E) {
            const bool done = (term[i] | trunc[i]) != 0;
            ret = io.run_return[i] + double(rew[i]);
            len = io.run_length[i] + 1;
            cnt = io.count[i];
            q = quota ? quota[i] : 0;
            f = done && (!quota || cnt < q);
        }
        const uint64_t b = __ballot(f);
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int c = wsum[w];
            off += w < wave ? c : 0;
            tot += c;
        }
        if (i < E) {
            if (f) {
                const int r = off + __popcll(b & ((uint64_t(1) << lane) - 1));
                const long long pos = total + r;
                long long slot = -1;
                if (io.ring) {
                    if (r >= first) slot = pos % C;
                } else if (pos < C) {
                    slot = pos;
                }
                if (slot >= 0) {
                    io.log_return[slot] = ret;
                    io.log_length[slot] = len;
                    io.log_env[slot] = i;
                }
                cnt += 1;
                io.count[i] = cnt;
                ret = 0.0;
                len = 0;
            }
            io.run_return[i] = ret;
            io.run_length[i] = len;
            if (quota && q > cnt) rem += q - cnt;
        }
        base += tot;
        __syncthreads();   // wsum is rewritten by the next chunk
    }

#pragma unroll
    for (int s = 32; s > 0; s >>= 1) rem += __shfl_down(rem, s);
    if (lane == 0) wrem[wave] = rem;
    __syncthreads();
    if (tid == 0) {
        long long r = 0;
        for (int w = 0; w < kWaves; ++w) r += wrem[w];
        const long long after = total + k;
        io.meta[0] = after;
        io.meta[1] = r;
        io.meta[2] += 1;
        if (!io.ring) io.meta[3] += (after > C ? after - C : 0) - (total > C ? total - C : 0);
    }
}

// Fixed-order workgroup reductions of one double per lane (LDS tree: the same pairs in the same order
// whatever the data).
template <int OP>
__device__ double block_reduce(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = kLanes / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double a = sh[tid], b = sh[tid + s];
            sh[tid] = OP == 0 ? a + b : OP == 1 ? fmin(a, b) : fmax(a, b);
        }
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();   // sh is reused by the next reduction
    return r;
}

// out8 = {n, mean return, std return (ddof 0), min, max, mean length, std length, total} over the
// n = min(total, C) logged episodes; two-pass variance in double.  n = 0: NaN (SB3 safe_mean).
__global__ void __launch_bounds__(kLanes) episode_summary_kernel(adrp_episode_io io, double* __restrict__ out8) {
    __shared__ double sh[kLanes];
    const int tid = threadIdx.x;
    const long long total = io.meta[0];
    const int n = total < io.capacity ? int(total) : io.capacity;
    double sr = 0.0, sl = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int j = tid; j < n; j += kLanes) {
        const double r = io.log_return[j];
        sr += r;
        sl += double(io.log_length[j]);
        mn = fmin(mn, r);
        mx = fmax(mx, r);
    }
    sr = block_reduce<0>(sr, sh);
    sl = block_reduce<0>(sl, sh);
    mn = block_reduce<1>(mn, sh);
    mx = block_reduce<2>(mx, sh);
    const double nan = __builtin_nan("");
    const double mr = n > 0 ? sr / n : nan, ml = n > 0 ? sl / n : nan;
    double vr = 0.0, vl = 0.0;
    for (int j = tid; j < n; j += kLanes) {
        const double dr = io.log_return[j] - mr, dl = double(io.log_length[j]) - ml;
        vr += dr * dr;
        vl += dl * dl;
    }
    vr = block_reduce<0>(vr, sh);
    vl = block_reduce<0>(vl, sh);
    if (tid == 0) {
        out8[0] = double(n);
        out8[1] = mr;
        out8[2] = n > 0 ? sqrt(vr / n) : nan;
        out8[3] = n > 0 ? mn : nan;
        out8[4] = n > 0 ? mx : nan;
        out8[5] = ml;
        out8[6] = n > 0 ? sqrt(vl / n) : nan;
        out8[7] = double(total);
    }
}

// the refusals shared by both entry points; returns nullptr when io is usable
const char* episode_io_error(const adrp_episode_io* io) {
    if (!io) return "io is NULL";
    if (io->struct_size != sizeof(adrp_episode_io)) return "adrp_episode_io.struct_size mismatch (ABI)";
    if (io->num_envs < 1) return "num_envs must be at least 1";
    if (io->capacity < 1) return "capacity must be at least 1";
    if (io->ring != 0 && io->ring != 1) return "ring must be 0 or 1";
    if (!io->run_return || !io->run_length || !io->count || !io->meta || !io->log_return || !io->log_length || !io->log_env)
        return "NULL buffer in adrp_episode_io (only quota may be NULL)";
    return nullptr;
}

}  // namespace

extern "C" int adrp_episode_step(const adrp_episode_io* io, const float* rew, const uint8_t* term, const uint8_t* trunc,
                                 void* stream) {
    if (const char* why = episode_io_error(io)) return seterr(nullptr, ADRP_ERR_INVALID, std::string("adrp_episode_step: ") + why);
    if (!rew || !term || !trunc) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_episode_step: NULL argument (rew / term / trunc)");
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(episode_step_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, *io, rew, term, trunc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("episode step launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}

extern "C" int adrp_episode_summary(const adrp_episode_io* io, double* out8, void* stream) {
    if (const char* why = episode_io_error(io)) return seterr(nullptr, ADRP_ERR_INVALID, std::string("adrp_episode_summary: ") + why);
    if (!out8) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_episode_summary: NULL argument (out8)");
    StreamDeviceGuard g((hipStream_t)stream);
    hipLaunchKernelGGL(episode_summary_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, *io, out8);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("episode summary launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}
