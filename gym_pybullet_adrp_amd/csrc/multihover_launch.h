// multihover_launch.h — MultiHoverAviary step/reset launchers (instantiated by multihover_f32.hip /
// multihover_f64.hip)
#pragma once

#include "adrp_internal.h"

template <typename Real, int PH, int A, int G, int B>
static void mh_launch_b(const HoverArgs<Real>& a, const MultiConst<Real>* m, hipStream_t s, adrp_t* h) {
    const long long lanes = (long long)h->E * G;
    const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock)), blk(kBlock);
    auto kernel = multihover_step_kernel<Real, PH, A, G, B>;
    if (h->prof_n < h->prof_cap) {
        hipExtLaunchKernelGGL(kernel, grid, blk, 0, s, h->ev_start[h->prof_n], h->ev_stop[h->prof_n], 0, a, m);
        ++h->prof_n;
    } else {
        hipLaunchKernelGGL(kernel, grid, blk, 0, s, a, m);
    }
}

// the reference's ring length (CTRL_FREQ 30: 15) has the ring in registers; any other is read at run time
template <typename Real, int PH, int A, int G>
static void mh_launch(const HoverArgs<Real>& a, const MultiConst<Real>* m, hipStream_t s, adrp_t* h) {
    if (h->B == 15) mh_launch_b<Real, PH, A, G, 15>(a, m, s, h);
    else mh_launch_b<Real, PH, A, G, 0>(a, m, s, h);
}

template <typename Real, int PH, int A>
static void mh_launch_g(const HoverArgs<Real>& a, const MultiConst<Real>* m, hipStream_t s, adrp_t* h) {
    switch (mh_group(h->N)) {
        case 1: mh_launch<Real, PH, A, 1>(a, m, s, h); break;
        case 2: mh_launch<Real, PH, A, 2>(a, m, s, h); break;
        case 4: mh_launch<Real, PH, A, 4>(a, m, s, h); break;
        default: mh_launch<Real, PH, A, 8>(a, m, s, h); break;
    }
}

template <typename Real, int A>
static void mh_launch_ph(const HoverArgs<Real>& a, const MultiConst<Real>* m, hipStream_t s, adrp_t* h) {
    switch (h->cfg.physics) {
        case ADRP_PHYS_PYB: mh_launch_g<Real, ADRP_PHYS_PYB, A>(a, m, s, h); break;
        case ADRP_PHYS_DYN: mh_launch_g<Real, ADRP_PHYS_DYN, A>(a, m, s, h); break;
        case ADRP_PHYS_PYB_GND: mh_launch_g<Real, ADRP_PHYS_PYB_GND, A>(a, m, s, h); break;
        case ADRP_PHYS_PYB_DRAG: mh_launch_g<Real, ADRP_PHYS_PYB_DRAG, A>(a, m, s, h); break;
        case ADRP_PHYS_PYB_DW: mh_launch_g<Real, ADRP_PHYS_PYB_DW, A>(a, m, s, h); break;
        default: mh_launch_g<Real, ADRP_PHYS_PYB_GND_DRAG_DW, A>(a, m, s, h); break;
    }
}

template <typename Real>
int multihover_step(adrp_t* h, const float* act, float* obs, float* rew, uint8_t* term, uint8_t* trunc, float* tobs,
                    hipStream_t s) {
    HoverArgs<Real> a = hover_args<Real>(h);
    a.act = act; a.obs = obs; a.rew = rew; a.term = term; a.trunc = trunc; a.tobs = tobs;
    const MultiConst<Real>* m = multihover_const<Real>(h);
    if (h->A == 1) mh_launch_ph<Real, 1>(a, m, s, h);
    else mh_launch_ph<Real, 4>(a, m, s, h);
    HIPCHK(h, hipGetLastError());
    return ADRP_OK;
}

template <typename Real>
int multihover_reset(adrp_t* h, const uint8_t* mask, float* obs, hipStream_t s) {
    HoverArgs<Real> a = hover_args<Real>(h);
    a.mask = mask; a.obs = obs;
    const MultiConst<Real>* m = multihover_const<Real>(h);
    const size_t EN = size_t(h->E) * h->N;
    const dim3 grid((unsigned)((EN + 255) / 256)), blk(256);
    if (h->A == 1) hipLaunchKernelGGL((multihover_reset_kernel<Real, 1>), grid, blk, 0, s, a, m);
    else hipLaunchKernelGGL((multihover_reset_kernel<Real, 4>), grid, blk, 0, s, a, m);
    HIPCHK(h, hipGetLastError());
    return ADRP_OK;
}
