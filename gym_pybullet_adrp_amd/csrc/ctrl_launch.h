// ctrl_launch.h — CtrlAviary / VelocityAviary step/reset launchers (instantiated by ctrl_f32.hip /
// ctrl_f64.hip)
#pragma once

#include "adrp_internal.h"

template <typename Real, int CTL>
static void ctrl_launch(const HoverArgs<Real>& a, const CtrlConst<Real>* k, const Real* rpm, hipStream_t s, adrp_t* h) {
    with_physics(h->cfg.physics, [&](auto ph) {
        with_group(h->N, [&](auto g) {
            constexpr int PH = decltype(ph)::value, G = decltype(g)::value;
            const long long lanes = (long long)h->E * G;
            const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock)), blk(kBlock);
            launch_profiled(h, ctrl_step_kernel<Real, PH, G, CTL>, grid, blk, s, a, k, rpm);
        });
    });
}

// act: float32 [E][N][4] (RPMs or velocity commands); rpm_real: CtrlAviary RPMs in the handle's own
// precision instead (adrp_step_rpm), act is then not read
template <typename Real>
int ctrl_step(adrp_t* h, const float* act, const void* rpm_real, float* obs, float* rew, uint8_t* term, uint8_t* trunc,
              hipStream_t s) {
    HoverArgs<Real> a = hover_args<Real>(h);
    a.act = act; a.obs = obs; a.rew = rew; a.term = term; a.trunc = trunc;
    const CtrlConst<Real>* k = ctrl_const<Real>(h);
    if (h->cfg.task == ADRP_TASK_VELOCITY) ctrl_launch<Real, ADRP_ACT_VEL>(a, k, (const Real*)nullptr, s, h);
    else ctrl_launch<Real, 0>(a, k, (const Real*)rpm_real, s, h);
    HIPCHK(h, hipGetLastError());
    return ADRP_OK;
}

template <typename Real>
int ctrl_reset(adrp_t* h, const uint8_t* mask, float* obs, hipStream_t s) {
    HoverArgs<Real> a = hover_args<Real>(h);
    a.mask = mask; a.obs = obs;
    const size_t EN = size_t(h->E) * h->N;
    const dim3 grid((unsigned)((EN + 255) / 256)), blk(256);
    hipLaunchKernelGGL(ctrl_reset_kernel<Real>, grid, blk, 0, s, a, ctrl_const<Real>(h));
    HIPCHK(h, hipGetLastError());
    return ADRP_OK;
}
