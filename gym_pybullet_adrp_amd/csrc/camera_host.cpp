// camera_host.cpp — the CPU twin of the drone camera (camera_core.h), a stand-alone program.
//
//   camera_host SCENE OUT
//
// SCENE: int32 header[16] = {E, N, W, H, G, O, gate_low[4], precision, cull, 0...}, then the state planes
//        of adrp_race_camera_io in that precision (0 float32, 1 float64): pos [3][E*N], quat [4][E*N],
//        gates [16][E*N], obstacles [12][E*N].
// OUT:   float32 dep[E*N][H][W], int32 seg[E*N][H][W], uint32 rgba[E*N][H][W], one block after the other.
// Built by `make camera_host` with the plain host compiler; tests/test_camera.py compares it with the numpy
// reference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "camera_core.h"

namespace {

constexpr int kHeader = 16, kPlanes = 3 + 4 + 16 + 12;

template <class T>
bool write_block(FILE* f, const std::vector<T>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <typename Real>
void render(const int32_t* hd, const Real* planes, std::vector<float>& dep, std::vector<int32_t>& seg,
            std::vector<uint32_t>& rgba) {
    using namespace adrp_cam;
    const int E = hd[0], N = hd[1], W = hd[2], H = hd[3];
    Scene<Real> sc;
    sc.N = N; sc.G = hd[4]; sc.O = hd[5];
    for (int g = 0; g < 4; ++g) sc.gate_low[g] = hd[6 + g] != 0;
    sc.EN = size_t(E) * N;
    sc.pos = planes; sc.quat = planes + 3 * sc.EN; sc.gates = planes + 7 * sc.EN; sc.obst = planes + 23 * sc.EN;
    const bool cull = hd[11] != 0;
    const int all = prim_count(N, sc.G, sc.O);
    Prim tab[kMaxPrims];
    for (size_t slot = 0; slot < sc.EN; ++slot) {
        const int n = int(slot % size_t(N));
        Real pos[3], q[4];
        load_pose(sc, slot, pos, q);
        const Cam cam = make_camera(pos, q);
        int count = 0;
        for (int k = 0; k < all; ++k) {
            float crel[3], bound;
            make_prim(sc, slot, n, k, pos, tab[count], crel, &bound);
            if (!cull || ball_in_view(cam, crel, bound)) ++count;
        }
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                const Pixel px = shade(cam, i, j, W, H, tab, count);
                const size_t at = (slot * H + i) * W + j;
                dep[at] = px.dep; seg[at] = px.seg; rgba[at] = px.rgba;
            }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: camera_host SCENE OUT\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t hd[kHeader];
    if (!f || std::fread(hd, sizeof(int32_t), kHeader, f) != size_t(kHeader)) {
        std::fprintf(stderr, "camera_host: %s has no int32 header[16]\n", argv[1]);
        if (f) std::fclose(f);
        return 2;
    }
    const bool ok_hd = hd[0] >= 1 && hd[1] >= 1 && hd[1] <= adrp_cam::kMaxDrones && hd[2] >= 1 && hd[3] >= 1 &&
                       hd[4] >= 0 && hd[4] <= adrp_cam::kMaxGates && hd[5] >= 0 && hd[5] <= adrp_cam::kMaxObst &&
                       (hd[10] == 0 || hd[10] == 1) && (long long)hd[0] * hd[1] * hd[2] * hd[3] <= (1LL << 26);
    if (!ok_hd) {
        std::fprintf(stderr, "camera_host: %s: header out of range (E, N, W, H, G, O, gate_low[4], precision, cull)\n", argv[1]);
        std::fclose(f);
        return 2;
    }
    const size_t EN = size_t(hd[0]) * hd[1], rs = hd[10] ? 8 : 4;
    std::vector<unsigned char> raw(kPlanes * EN * rs + 1);
    const size_t got = std::fread(raw.data(), 1, raw.size(), f);
    std::fclose(f);
    if (got != kPlanes * EN * rs) {
        std::fprintf(stderr, "camera_host: %s does not hold [35][E*N] state planes after the header\n", argv[1]);
        return 2;
    }
    const size_t px = EN * size_t(hd[2]) * hd[3];
    std::vector<float> dep(px);
    std::vector<int32_t> seg(px);
    std::vector<uint32_t> rgba(px);
    if (hd[10]) {
        std::vector<double> planes(kPlanes * EN);
        std::memcpy(planes.data(), raw.data(), planes.size() * sizeof(double));
        render<double>(hd, planes.data(), dep, seg, rgba);
    } else {
        std::vector<float> planes(kPlanes * EN);
        std::memcpy(planes.data(), raw.data(), planes.size() * sizeof(float));
        render<float>(hd, planes.data(), dep, seg, rgba);
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) {
        std::fprintf(stderr, "camera_host: cannot write %s\n", argv[2]);
        return 2;
    }
    const bool ok = write_block(o, dep) && write_block(o, seg) && write_block(o, rgba);
    if (std::fclose(o) != 0 || !ok) {
        std::fprintf(stderr, "camera_host: short write to %s\n", argv[2]);
        return 2;
    }
    return 0;
}
