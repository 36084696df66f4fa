// ctrl_launch.h — CtrlAviary / VelocityAviary step/reset launchers (instantiated by ctrl_f32.hip /
// ctrl_f64.hip)
#pragma once

#include "adrp_internal.h"

template <typename Real, int PH, int G, int CTL>
static void ctrl_launch(const HoverArgs<Real>& a, const CtrlConst<Real>* k, const Real* rpm, hipStream_t s, adrp_t* h) {
    const long long lanes = (long long)h->E * G;
    const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock)), blk(kBlock);
    auto kernel = ctrl_step_kernel<Real, PH, G, CTL>;
    if (h->prof_n < h->prof_cap) {
        hipExtLaunchKernelGGL(kernel, grid, blk, 0, s, h->ev_start[h->prof_n], h->ev_stop[h->prof_n], 0, a, k, rpm);
        ++h->prof_n;
    } else {
        hipLaunchKernelGGL(kernel, grid, blk, 0, s, a, k, rpm);
    }
}

template <typename Real, int PH, int CTL>
static void ctrl_launch_g(const HoverArgs<Real>& a, const CtrlConst<Real>* k, const Real* rpm, hipStream_t s, adrp_t* h) {
    switch (mh_group(h->N)) {
        case 1: ctrl_launch<Real, PH, 1, CTL>(a, k, rpm, s, h); break;
        case 2: ctrl_launch<Real, PH, 2, CTL>(a, k, rpm, s, h); break;
        case 4: ctrl_launch<Real, PH, 4, CTL>(a, k, rpm, s, h); break;
        default: ctrl_launch<Real, PH, 8, CTL>(a, k, rpm, s, h); break;
    }
}

template <typename Real, int CTL>
static void ctrl_launch_ph(const HoverArgs<Real>& a, const CtrlConst<Real>* k, const Real* rpm, hipStream_t s, adrp_t* h) {
    switch (h->cfg.physics) {
        case ADRP_PHYS_PYB: ctrl_launch_g<Real, ADRP_PHYS_PYB, CTL>(a, k, rpm, s, h); break;
        case ADRP_PHYS_DYN: ctrl_launch_g<Real, ADRP_PHYS_DYN, CTL>(a, k, rpm, s, h); break;
        case ADRP_PHYS_PYB_GND: ctrl_launch_g<Real, ADRP_PHYS_PYB_GND, CTL>(a, k, rpm, s, h); break;
        case ADRP_PHYS_PYB_DRAG: ctrl_launch_g<Real, ADRP_PHYS_PYB_DRAG, CTL>(a, k, rpm, s, h); break;
        case ADRP_PHYS_PYB_DW: ctrl_launch_g<Real, ADRP_PHYS_PYB_DW, CTL>(a, k, rpm, s, h); break;
        default: ctrl_launch_g<Real, ADRP_PHYS_PYB_GND_DRAG_DW, CTL>(a, k, rpm, s, h); break;
    }
}

// act: float32 [E][N][4] (RPMs or velocity commands); rpm_real: CtrlAviary RPMs in the handle's own
// precision instead (adrp_step_rpm), act is then not read
template <typename Real>
int ctrl_step(adrp_t* h, const float* act, const void* rpm_real, float* obs, float* rew, uint8_t* term, uint8_t* trunc,
              hipStream_t s) {
    HoverArgs<Real> a = hover_args<Real>(h);
    a.act = act; a.obs = obs; a.rew = rew; a.term = term; a.trunc = trunc;
    const CtrlConst<Real>* k = ctrl_const<Real>(h);
    if (h->cfg.task == ADRP_TASK_VELOCITY) ctrl_launch_ph<Real, ADRP_ACT_VEL>(a, k, nullptr, s, h);
    else ctrl_launch_ph<Real, 0>(a, k, (const Real*)rpm_real, s, h);
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
