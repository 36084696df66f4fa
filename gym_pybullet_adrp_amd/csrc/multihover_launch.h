// multihover_launch.h — MultiHoverAviary step/reset launchers (instantiated by multihover_f32.hip /
// multihover_f64.hip)
#pragma once

#include "adrp_internal.h"

// the reference's ring length (CTRL_FREQ 30: 15) has the ring in registers; any other is read at run time
template <typename Real, int A>
static void mh_launch(const HoverArgs<Real>& a, const MultiConst<Real>* m, hipStream_t s, adrp_t* h) {
    with_physics(h->cfg.physics, [&](auto ph) {
        with_group(h->N, [&](auto g) {
            constexpr int PH = decltype(ph)::value, G = decltype(g)::value;
            const long long lanes = (long long)h->E * G;
            const dim3 grid((unsigned)((lanes + kBlock - 1) / kBlock)), blk(kBlock);
            if (h->B == 15) launch_profiled(h, multihover_step_kernel<Real, PH, A, G, 15>, grid, blk, s, a, m);
            else launch_profiled(h, multihover_step_kernel<Real, PH, A, G, 0>, grid, blk, s, a, m);
        });
    });
}

template <typename Real>
int multihover_step(adrp_t* h, const float* act, float* obs, float* rew, uint8_t* term, uint8_t* trunc, float* tobs,
                    hipStream_t s) {
    HoverArgs<Real> a = hover_args<Real>(h);
    a.act = act; a.obs = obs; a.rew = rew; a.term = term; a.trunc = trunc; a.tobs = tobs;
    const MultiConst<Real>* m = multihover_const<Real>(h);
    if (h->A == 1) mh_launch<Real, 1>(a, m, s, h);
    else mh_launch<Real, 4>(a, m, s, h);
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
