// camera_kernel.h — the drone camera's launch (camera_core.h per pixel; include/adrp.h adrp_race_camera).
//
// One workgroup of 256 lanes per (env, drone).  Phase 1: wave 0 forms the view (in the state's precision;
// lane 0 hands it to the other waves through LDS) and its lanes each place one primitive of
// the env (up to 35) relative to the drone's eye, drop those whose bounding ball cannot reach
// into the view pyramid, and write the kept ones, in table order, into LDS (a ballot gives each its
// place: no atomics); one barrier.  Phase 2: lane l takes pixels l, l + 256, ...; every lane reads the
// same table entry at a time (an LDS broadcast) and issues one coalesced store per output plane, the
// rgba as one 32-bit word.  A block whose (env, drone) is masked out or off the capture schedule returns
// before any other load.
#pragma once

#include <hip/hip_runtime.h>

#include "camera_core.h"

namespace adrp_cam {

constexpr int kCamLanes = 256;

template <typename Real>
struct CamArgs {
    Scene<Real> sc;
    int width, height, capture_freq;
    const int32_t* step_counter;    // [E*N] or null
    const uint8_t* mask;            // [E] or null
    float* dep;                     // [E*N][H][W] or null
    int32_t* seg;
    uint32_t* rgb;
};

template <typename Real>
__global__ __launch_bounds__(kCamLanes) void race_camera_kernel(const CamArgs<Real> a) {
    const size_t slot = blockIdx.x;
    const int N = a.sc.N;
    const int e = int(slot / size_t(N)), n = int(slot - size_t(e) * N);
    if (a.mask && a.mask[e] == 0) return;
    if (a.capture_freq > 0 && a.step_counter[slot] % a.capture_freq != 0) return;

    __shared__ Prim tab[kMaxPrims];
    __shared__ Cam view;
    __shared__ int tab_n;
    const int tid = threadIdx.x;
    if (tid < 64) {
        Real pos[3], q[4];
        load_pose(a.sc, slot, pos, q);
        const Cam cam = make_camera(pos, q);
        if (tid == 0) view = cam;
        const int count = prim_count(N, a.sc.G, a.sc.O);
        Prim p;
        bool keep = false;
        if (tid < count) {
            float crel[3], bound;
            make_prim(a.sc, slot, n, tid, pos, p, crel, &bound);
            keep = ball_in_view(cam, crel, bound);
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) tab[__popcll(kept & ((1ull << tid) - 1ull))] = p;
        if (tid == 0) tab_n = __popcll(kept);
    }
    __syncthreads();
    const Cam cam = view;
    const int count = tab_n;
    const int W = a.width, HW = a.width * a.height;
    const size_t base = slot * size_t(HW);
    for (int pix = tid; pix < HW; pix += kCamLanes) {
        const int i = pix / W, j = pix - i * W;
        const Pixel px = shade(cam, i, j, W, a.height, tab, count);
        if (a.dep) a.dep[base + pix] = px.dep;
        if (a.seg) a.seg[base + pix] = px.seg;
        if (a.rgb) a.rgb[base + pix] = px.rgba;
    }
}

}  // namespace adrp_cam
