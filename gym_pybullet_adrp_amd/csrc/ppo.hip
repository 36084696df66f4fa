// ppo.hip — C-ABI of the on-device PPO update (include/adrp.h: adrp_ppo_*).
//
// Replaces, for a policy resident on the GPU, stable_baselines3 2.3.2 PPO.train()'s inner loop body
// (examples/learn.py:72-94 reaches it through model.learn): evaluate_actions, the clipped surrogate
// loss, loss.backward(), clip_grad_norm_ and optimizer.step() on one minibatch, in four launches on
// the caller's stream (csrc/ppo_kernel.h), the updated weights written back into the policy's
// fragment blobs in place.
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>

#include "../../include/adrp.h"
#define ADRP_PPO_SMALL_KERNELS
#include "ppo_kernel.h"
#include "policy_handle.h"
#include "device_guard.h"

using namespace adrp;

int seterr(adrp_t* h, int code, const std::string& msg);

struct adrp_ppo {
    adrp_policy_t* policy = nullptr;
    adrp_ppo_cfg cfg{};
    PpoDesc d{};
    int total = 0;           // floats in the flat parameter vector
    int max_blocks = 0;      // partial slabs
    int nparts = 0;          // squared-norm partials (reduce blocks, 64 parameters each)
    int pblocks = 0;         // blocks of the one-thread-per-parameter kernels
    float* params = nullptr; // master parameters, Adam's m, v, the raw gradient: [total] each
    float* m = nullptr;
    float* v = nullptr;
    float* grad = nullptr;
    float* partial = nullptr;
    float* spart = nullptr;
    double* advpart = nullptr;
    float* stats = nullptr;  // where the statistics go when the caller passes no stats_out
    double* normpart = nullptr;
    int* t = nullptr;
    int* stop = nullptr;     // the target_kl latch (ppo_kernel.h): tripped, steps applied, tripped as Adam saw it, spare
    bool kl_on = false;      // adrp_ppo_set_target_kl
    double kl_thr = 0.0;     // 1.5 * target_kl
    float* images = nullptr; // w2t / w3t of both nets
};

extern "C" int adrp_ppo_default_cfg(adrp_ppo_cfg* c) {
    if (!c) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_default_cfg: cfg is NULL");
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(adrp_ppo_cfg);
    c->normalize_advantage = 1;
    c->learning_rate = 3e-4;
    c->clip_range = 0.2;
    c->clip_range_vf = -1.0;
    c->ent_coef = 0.0;
    c->vf_coef = 0.5;
    c->max_grad_norm = 0.5;
    return ADRP_OK;
}

static void ppo_free(adrp_ppo_t* q) {
    hipFree(q->params); hipFree(q->m); hipFree(q->v); hipFree(q->grad); hipFree(q->partial); hipFree(q->spart);
    hipFree(q->advpart); hipFree(q->stats); hipFree(q->normpart); hipFree(q->t); hipFree(q->stop); hipFree(q->images);
    delete q;
}

extern "C" int adrp_ppo_create(adrp_policy_t* p, const adrp_ppo_cfg* cfg, adrp_ppo_t** out) {
    if (!out) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_create: out is NULL");
    *out = nullptr;
    // every refusal before any device call
    if (!cfg || cfg->struct_size != sizeof(adrp_ppo_cfg))
        return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_create: cfg is NULL or its struct_size is not sizeof(adrp_ppo_cfg)");
    if (!(cfg->learning_rate > 0.0)) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_create: learning_rate must be positive");
    if (!(cfg->clip_range >= 0.0)) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_create: clip_range must not be negative");
    if (!p) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_create: policy is NULL");
    if (!p->critic || !p->log_std)
        return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_create: the policy has no critic (adrp_policy_set_critic)");
    adrp_ppo_t* q = new adrp_ppo_t();
    q->policy = p;
    q->cfg = *cfg;
    PpoDesc& d = q->d;
    d.in_dim = p->in_dim; d.h1 = p->h1; d.h2 = p->h2; d.act_dim = p->act_dim;
    d.L[0] = p->L; d.L[1] = p->Lc;
    d.blob[0] = p->blob; d.blob[1] = p->critic; d.log_std = p->log_std;
    int o = 0;
    for (int net = 0; net < 2; ++net) {
        const int n_out = net ? 1 : p->act_dim;
        const int sizes[6] = {p->h1 * p->in_dim, p->h1, p->h2 * p->h1, p->h2, n_out * p->h2, n_out};
        for (int k = 0; k < 6; ++k) { d.off[6 * net + k] = o; o += sizes[k]; }
    }
    d.off[12] = o; o += p->act_dim;
    d.off[13] = o;
    q->total = o;
    q->nparts = (o + 63) / 64;
    q->pblocks = (o + 255) / 256;
    // slabs: at most 64 MiB of them, 8..256 blocks
    int mb = int((size_t(16) << 20) / size_t(o));
    q->max_blocks = mb < 8 ? 8 : (mb > 256 ? 256 : mb);
    const int T1 = p->h1 / 16, T2 = p->h2 / 16;
    const size_t w2t_n = size_t(T1) * T2 * 256, w3t_n[2] = {size_t(T2) * d.L[0].t3 * 256, size_t(T2) * d.L[1].t3 * 256};
    const size_t img_n = 2 * w2t_n + w3t_n[0] + w3t_n[1];

    DeviceGuard g(p->device);
    const size_t fb = size_t(o) * sizeof(float);
    bool ok = hipMalloc((void**)&q->params, fb) == hipSuccess && hipMalloc((void**)&q->m, fb) == hipSuccess &&
              hipMalloc((void**)&q->v, fb) == hipSuccess && hipMalloc((void**)&q->grad, fb) == hipSuccess &&
              hipMalloc((void**)&q->partial, fb * q->max_blocks) == hipSuccess &&
              hipMalloc((void**)&q->spart, sizeof(float) * 4 * q->max_blocks) == hipSuccess &&
              hipMalloc((void**)&q->advpart, sizeof(double) * 2 * kPpoAdvBlocks) == hipSuccess &&
              hipMalloc((void**)&q->stats, sizeof(float) * 8) == hipSuccess &&
              hipMalloc((void**)&q->normpart, sizeof(double) * q->nparts) == hipSuccess &&
              hipMalloc((void**)&q->t, sizeof(int)) == hipSuccess &&
              hipMalloc((void**)&q->stop, sizeof(int) * 4) == hipSuccess &&
              hipMalloc((void**)&q->images, sizeof(float) * img_n) == hipSuccess;
    if (!ok) {
        ppo_free(q);
        return seterr(nullptr, ADRP_ERR_OOM, "adrp_ppo_create: hipMalloc failed");
    }
    d.w2t[0] = q->images;
    d.w2t[1] = d.w2t[0] + w2t_n;
    d.w3t[0] = d.w2t[1] + w2t_n;
    d.w3t[1] = d.w3t[0] + w3t_n[0];
    ok = hipMemset(q->m, 0, fb) == hipSuccess && hipMemset(q->v, 0, fb) == hipSuccess &&
         hipMemset(q->grad, 0, fb) == hipSuccess && hipMemset(q->t, 0, sizeof(int)) == hipSuccess &&
         hipMemset(q->stop, 0, sizeof(int) * 4) == hipSuccess &&
         hipMemset(q->images, 0, sizeof(float) * img_n) == hipSuccess;   // W3's rows beyond n_out stay zero
    if (ok) {   // the master parameters are what the policy's blobs hold
        hipLaunchKernelGGL(ppo_pack_kernel, dim3(q->pblocks), dim3(256), 0, nullptr, d, q->params, 1);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) {
        ppo_free(q);
        return seterr(nullptr, ADRP_ERR_DEVICE, "adrp_ppo_create: device initialisation failed");
    }
    *out = q;
    return ADRP_OK;
}

extern "C" void adrp_ppo_destroy(adrp_ppo_t* q) {
    if (!q) return;
    DeviceGuard g(q->policy->device);
    hipDeviceSynchronize();
    ppo_free(q);
}

extern "C" int adrp_ppo_param_count(const adrp_ppo_t* q) {
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_param_count: ppo is NULL");
    return q->total;
}

extern "C" int adrp_ppo_update(adrp_ppo_t* q, const float* obs, int obs_stride, const float* actions, const float* old_values,
                               const float* old_log_prob, const float* advantages, const float* returns, const int64_t* idx,
                               int n, float* stats_out, void* stream) {
    if (n < 1) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_update: n must be at least 1");
    if (!q || !obs || !actions || !old_values || !old_log_prob || !advantages || !returns || !idx)
        return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_update: NULL argument");
    if (obs_stride < q->d.in_dim) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_update: obs_stride < in_dim");
    const adrp_policy_t* p = q->policy;
    const int T1 = p->h1 / 16;
    const int rg_max = T1 >= 8 ? 2 : (T1 == 4 ? 4 : 8);  // ppo_group_tiles<T1>()
    // as many blocks as there are slabs before a block takes a second row tile: one tile's chain of
    // barriers is what a small minibatch costs; groups only bound the number of slabs
    const int tiles = (n + 15) / 16;
    int rg = (tiles + q->max_blocks - 1) / q->max_blocks;
    rg = rg < 1 ? 1 : (rg > rg_max ? rg_max : rg);
    const int ngroups = (tiles + rg - 1) / rg;
    const int grid = ngroups < q->max_blocks ? ngroups : q->max_blocks;
    PpoGradArgs a;
    a.d = q->d;
    a.obs = obs; a.obs_stride = obs_stride; a.actions = actions;
    a.old_values = old_values; a.old_log_prob = old_log_prob; a.adv = advantages; a.ret = returns;
    const bool norm = q->cfg.normalize_advantage && n > 1;
    a.idx = idx; a.n = n; a.advpart = norm ? q->advpart : nullptr;
    a.clip = float(q->cfg.clip_range); a.clip_vf = float(q->cfg.clip_range_vf); a.vf_coef = float(q->cfg.vf_coef);
    a.partial = q->partial; a.spart = q->spart; a.ngroups = ngroups; a.rg = rg;
    a.stop = q->stop;
    DeviceGuard g(p->device);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (norm) {
        hipLaunchKernelGGL(ppo_advstat_kernel, dim3(kPpoAdvBlocks), dim3(256), 0, s, advantages, idx, n, q->advpart, q->stop);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = p->relu ? ppo_grad_launch_relu(p->h1, p->h2, a, grid, s) : ppo_grad_launch_tanh(p->h1, p->h2, a, grid, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ppo_reduce_kernel, dim3(q->nparts), dim3(256), 0, s, q->partial, grid, q->total, q->d.off[12],
                           float(q->cfg.ent_coef), q->grad, q->normpart, q->spart, n, q->d.log_std, q->d.act_dim,
                           stats_out ? stats_out : q->stats, q->t, q->stop, q->kl_on ? 1 : 0, q->kl_thr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ppo_adam_kernel, dim3(q->pblocks), dim3(256), 0, s, q->d, q->grad, q->normpart, q->nparts, q->params,
                           q->m, q->v, q->t, q->cfg.learning_rate, q->cfg.max_grad_norm, q->stop);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("ppo update launch: ") + hipGetErrorString(e));
    return ADRP_OK;
}

extern "C" int adrp_ppo_set_target_kl(adrp_ppo_t* q, double target_kl) {
    // (the values before the handle, as adrp_ppo_create checks its cfg before its policy: every refusal answers without a device)
    if (target_kl != target_kl) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_target_kl: target_kl is NaN");
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_target_kl: ppo is NULL");
    q->kl_on = target_kl >= 0.0;
    q->kl_thr = q->kl_on ? 1.5 * target_kl : 0.0;
    return ADRP_OK;
}

extern "C" int adrp_ppo_set_rates(adrp_ppo_t* q, double learning_rate, double clip_range, double clip_range_vf) {
    if (!(learning_rate > 0.0)) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_rates: learning_rate must be positive");
    if (!(clip_range >= 0.0)) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_rates: clip_range must not be negative");
    if (clip_range_vf != clip_range_vf) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_rates: clip_range_vf is NaN");
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_rates: ppo is NULL");
    q->cfg.learning_rate = learning_rate;
    q->cfg.clip_range = clip_range;
    q->cfg.clip_range_vf = clip_range_vf;
    return ADRP_OK;
}

extern "C" int adrp_ppo_train_begin(adrp_ppo_t* q, void* stream) {
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_train_begin: ppo is NULL");
    DeviceGuard g(q->policy->device);
    if (hipMemsetAsync(q->stop, 0, sizeof(int) * 4, (hipStream_t)stream) != hipSuccess)
        return seterr(nullptr, ADRP_ERR_DEVICE, "adrp_ppo_train_begin: memset failed");
    return ADRP_OK;
}

extern "C" int adrp_ppo_stop_state(adrp_ppo_t* q, int32_t* out_dev2, void* stream) {
    if (!out_dev2) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_stop_state: out_dev2 is NULL");
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_stop_state: ppo is NULL");
    DeviceGuard g(q->policy->device);
    if (hipMemcpyAsync(out_dev2, q->stop, 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return seterr(nullptr, ADRP_ERR_DEVICE, "adrp_ppo_stop_state: copy failed");
    return ADRP_OK;
}

static hipError_t copy_f(void* dst, const void* src, size_t bytes, hipStream_t s) {
    return (dst && src) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
}

extern "C" int adrp_ppo_params(adrp_ppo_t* q, float* params_out, float* m_out, float* v_out, int32_t* t_out, void* stream) {
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_params: ppo is NULL");
    DeviceGuard g(q->policy->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t fb = size_t(q->total) * sizeof(float);
    if (copy_f(params_out, q->params, fb, s) != hipSuccess || copy_f(m_out, q->m, fb, s) != hipSuccess ||
        copy_f(v_out, q->v, fb, s) != hipSuccess || copy_f(t_out, q->t, sizeof(int32_t), s) != hipSuccess)
        return seterr(nullptr, ADRP_ERR_DEVICE, "adrp_ppo_params: copy failed");
    return ADRP_OK;
}

extern "C" int adrp_ppo_set_params(adrp_ppo_t* q, const float* params, const float* m, const float* v, int t, void* stream) {
    if (!q) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_set_params: ppo is NULL");
    DeviceGuard g(q->policy->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t fb = size_t(q->total) * sizeof(float);
    hipError_t e = copy_f(q->params, params, fb, s);
    if (e == hipSuccess) e = copy_f(q->m, m, fb, s);
    if (e == hipSuccess) e = copy_f(q->v, v, fb, s);
    if (e == hipSuccess && t >= 0) e = hipMemsetD32Async((hipDeviceptr_t)q->t, t, 1, s);
    if (e == hipSuccess && params) {
        hipLaunchKernelGGL(ppo_pack_kernel, dim3(q->pblocks), dim3(256), 0, s, q->d, q->params, 0);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return seterr(nullptr, ADRP_ERR_DEVICE, std::string("adrp_ppo_set_params: ") + hipGetErrorString(e));
    return ADRP_OK;
}

extern "C" int adrp_ppo_gradients(adrp_ppo_t* q, float* grad_out, void* stream) {
    if (!q || !grad_out) return seterr(nullptr, ADRP_ERR_INVALID, "adrp_ppo_gradients: NULL argument");
    DeviceGuard g(q->policy->device);
    if (copy_f(grad_out, q->grad, size_t(q->total) * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return seterr(nullptr, ADRP_ERR_DEVICE, "adrp_ppo_gradients: copy failed");
    return ADRP_OK;
}
