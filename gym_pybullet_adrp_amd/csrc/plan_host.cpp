// plan_host.cpp — the CPU twin of the device spline planner (spline_plan.h), a stand-alone program.
//
//   plan_host CASES SAMPLES OUT
//
// CASES:   raw float64 [cases][10]: start x, y, then the four nominal gates' x, y.
// SAMPLES: raw float64 [L]: the parameter values of splev (np.linspace(0, 1, L)).
// OUT:     int32 n[cases], int32 status[cases], float64 t[cases][20], float64 c[cases][3][16],
//          float64 ref[cases][L][3], one block after the other.
// Built by `make plan_host` with the plain host compiler; tests/test_plan.py compares it with scipy.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "spline_plan.h"

namespace {

bool read_doubles(const char* path, std::vector<double>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % long(sizeof(double)) != 0) {
        std::fclose(f);
        return false;
    }
    out.resize(size_t(bytes) / sizeof(double));
    const size_t got = out.empty() ? 0 : std::fread(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return got == out.size();
}

template <class T>
bool write_block(FILE* f, const std::vector<T>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

}  // namespace

int main(int argc, char** argv) {
    using namespace adrp_plan;
    constexpr int M = kHardPoints, NT = M + kK1;
    if (argc != 4) {
        std::fprintf(stderr, "usage: plan_host CASES SAMPLES OUT\n");
        return 2;
    }
    std::vector<double> cases, samples;
    if (!read_doubles(argv[1], cases) || cases.empty() || cases.size() % 10 != 0) {
        std::fprintf(stderr, "plan_host: %s is not a float64 [cases][10] file\n", argv[1]);
        return 2;
    }
    if (!read_doubles(argv[2], samples) || samples.size() < 2) {
        std::fprintf(stderr, "plan_host: %s is not a float64 [L >= 2] file\n", argv[2]);
        return 2;
    }
    const size_t C = cases.size() / 10, L = samples.size();
    std::vector<int32_t> n(C), status(C);
    std::vector<double> t(C * NT), c(C * kDim * M), ref(C * L * 3);
    Work<M> work;
    Spline<M> sp;
    double w[M * 3];
    for (size_t i = 0; i < C; ++i) {
        const double* in = &cases[i * 10];
        hardcoded_waypoints(in[0], in[1], in + 2, w);
        smoothing_fit<M>(w, kHardSmooth, work, sp);
        int flags = sp.flags;
        for (int j = 0; j < NT; ++j) t[i * NT + j] = sp.t[j];
        for (int d = 0; d < kDim; ++d)
            for (int j = 0; j < M; ++j) c[(i * kDim + d) * M + j] = sp.c[d][j];
        for (size_t j = 0; j < L; ++j) {
            double* out = &ref[(i * L + j) * 3];
            spline_eval(sp.t, &sp.c[0][0], M, sp.n, samples[j], out);
            if (!(out[2] < kCeiling)) flags |= kStatCeiling;
        }
        n[i] = sp.n;
        status[i] = status_word(flags, sp.n, sp.iters);
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) {
        std::fprintf(stderr, "plan_host: cannot write %s\n", argv[3]);
        return 2;
    }
    const bool ok = write_block(f, n) && write_block(f, status) && write_block(f, t) && write_block(f, c) && write_block(f, ref);
    if (std::fclose(f) != 0 || !ok) {
        std::fprintf(stderr, "plan_host: short write to %s\n", argv[3]);
        return 2;
    }
    return 0;
}
