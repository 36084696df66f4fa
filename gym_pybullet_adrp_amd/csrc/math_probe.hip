// math_probe.hip — adrp_math_probe: evaluates the fp64 fast transcendentals of adrp_device.h
// (namespace f64, the exp-map forms, the race noise Box-Muller) over a device array, so
// tests/test_math_gpu.py can check them against extended-precision references and the oracle (the
// step kernels inline the same functions); adrp_math_probe_v does the same for the Euler-angle /
// quaternion conversions and the fp32 fast forms, in float and double.  This TU compiles with the race
// TUs' contraction mode (hipcc's default), so it stands in for them, not for the hover TUs.
#include <hip/hip_runtime.h>

#include "adrp_device.h"
#include "../../include/adrp.h"

namespace {
__global__ void __launch_bounds__(256) math_probe_kernel(int fn, const double* __restrict__ in, double* __restrict__ out,
                                                         int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    double r = 0.0, c = 0.0;
    switch (fn) {
        case ADRP_MATH_RCP: r = adrp::f64::rcp(x); break;
        case ADRP_MATH_RSQ: r = adrp::f64::rsq(x); break;
        case ADRP_MATH_SQRT: r = adrp::f64::sqrt(x); break;
        case ADRP_MATH_SIN_SMALL: adrp::f64::sincos_small(x, &r, &c); break;
        case ADRP_MATH_COS_SMALL: adrp::f64::sincos_small(x, &c, &r); break;
        case ADRP_MATH_ATAN2: r = adrp::f64::atan2(x, in[n + i]); break;
        case ADRP_MATH_ASIN: r = adrp::f64::asin(x); break;
        case ADRP_MATH_EXP: r = adrp::f64::exp(x); break;
        case ADRP_MATH_SQRT_NN: r = adrp::f64::sqrt_nn(x); break;
        case ADRP_MATH_RCP_NC: r = adrp::f64::rcp_nc(x); break;
        case ADRP_MATH_RSQ_NC: r = adrp::f64::rsq_nc(x); break;
        case ADRP_MATH_SIN_TINY: adrp::f64::sincos_tiny(x, &r, &c); break;
        case ADRP_MATH_COS_TINY: adrp::f64::sincos_tiny(x, &c, &r); break;
        case ADRP_MATH_EXPMAP_SINC: adrp::expmap_sinc_cos(x, &r, &c); break;
        case ADRP_MATH_EXPMAP_COS: adrp::expmap_sinc_cos(x, &c, &r); break;
        case ADRP_MATH_QUAT_INV_NORM: r = adrp::quat_inv_norm(x); break;
        case ADRP_MATH_DIVC: r = adrp::f64::div_c(x, in[n + i]); break;
        case ADRP_MATH_SIN_FAST: adrp::f64::sincos_fast(x, &r, &c); break;
        case ADRP_MATH_COS_FAST: adrp::f64::sincos_fast(x, &c, &r); break;
        case ADRP_MATH_EXP_TAB: r = adrp::f64::exp_tab(x, adrp::f64::kExp2Tab32); break;
        case ADRP_MATH_ATAN2_NC: r = adrp::f64::atan2_nc(x, in[n + i]); break;
        case ADRP_MATH_FDIV_RCP: r = adrp::f64::fdiv_rcp(float(x), adrp::f64::rcp(double(float(in[n + i])))); break;
        case ADRP_MATH_NORMAL_Z0:
        case ADRP_MATH_NORMAL_Z1: {
            const unsigned long long b = (unsigned long long)__double_as_longlong(x);
            float z0, z1;
            adrp::normal_pair_f(uint32_t(b), uint32_t(b >> 32), &z0, &z1);
            r = fn == ADRP_MATH_NORMAL_Z0 ? z0 : z1;
            break;
        }
        default: r = __builtin_nan(""); break;
    }
    out[i] = r;
}

// adrp_math_probe_v: the attitude forms and the fp32 fast forms, in Real = float or double, on planes
// in[k][n] -> out[m][n] (doubles on the wire; a float instantiation rounds its inputs to float, which
// is exact for the float-representable values the tests send, and widens its results exactly).
// One lane per column, 64-lane waves in column order, so a test chooses which columns share a
// wave-uniform vote (euler_xyz_fast_u, clamp100_wv).
template <typename Real>
__global__ void __launch_bounds__(256) math_probe_v_kernel(int fn, const double* __restrict__ in, double* __restrict__ out,
                                                           int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto ld = [&](int k) { return Real(in[size_t(k) * n + i]); };
    auto st = [&](int k, Real v) { out[size_t(k) * n + i] = double(v); };
    switch (fn) {
        case ADRP_MATHV_EULER_XYZ:
        case ADRP_MATHV_EULER_XYZ_FAST:
        case ADRP_MATHV_EULER_XYZ_FAST_U: {
            const adrp::Q4<Real> q{ld(0), ld(1), ld(2), ld(3)};
            const adrp::V3<Real> e = fn == ADRP_MATHV_EULER_XYZ        ? adrp::euler_xyz(q)
                                     : fn == ADRP_MATHV_EULER_XYZ_FAST ? adrp::euler_xyz_fast(q)
                                                                       : adrp::euler_xyz_fast_u(q);
            st(0, e.x); st(1, e.y); st(2, e.z);
            break;
        }
        case ADRP_MATHV_QUAT_FROM_EULER:
        case ADRP_MATHV_QUAT_FROM_EULER_FAST: {
            const adrp::Q4<Real> q = fn == ADRP_MATHV_QUAT_FROM_EULER ? adrp::quat_from_euler(ld(0), ld(1), ld(2))
                                                                      : adrp::quat_from_euler_fast(ld(0), ld(1), ld(2));
            st(0, q.x); st(1, q.y); st(2, q.z); st(3, q.w);
            break;
        }
        case ADRP_MATHV_FATAN2: st(0, adrp::fatan2_(ld(0), ld(1))); break;
        case ADRP_MATHV_FASIN: st(0, adrp::fasin_(ld(0))); break;
        case ADRP_MATHV_FEXP: st(0, adrp::fexp_(ld(0))); break;
        case ADRP_MATHV_SMALL_SINCOS: {
            Real s, c;
            adrp::small_sincos(ld(0), &s, &c);
            st(0, s); st(1, c);
            break;
        }
        case ADRP_MATHV_EXPMAP_SINC_COS: {
            Real s, c;
            adrp::expmap_sinc_cos(ld(0), &s, &c);
            st(0, s); st(1, c);
            break;
        }
        case ADRP_MATHV_QUAT_INV_NORM: st(0, adrp::quat_inv_norm(ld(0))); break;
        case ADRP_MATHV_CLAMP100_WV: {
            adrp::V3<Real> w{ld(0), ld(1), ld(2)}, v{ld(3), ld(4), ld(5)};
            adrp::clamp100_wv(w, v);
            st(0, w.x); st(1, w.y); st(2, w.z); st(3, v.x); st(4, v.y); st(5, v.z);
            break;
        }
        default: break;
    }
}

bool mathv_planes(int fn, int* k_in, int* k_out) {
    switch (fn) {
        case ADRP_MATHV_EULER_XYZ:
        case ADRP_MATHV_EULER_XYZ_FAST:
        case ADRP_MATHV_EULER_XYZ_FAST_U: *k_in = 4; *k_out = 3; return true;
        case ADRP_MATHV_QUAT_FROM_EULER:
        case ADRP_MATHV_QUAT_FROM_EULER_FAST: *k_in = 3; *k_out = 4; return true;
        case ADRP_MATHV_FATAN2: *k_in = 2; *k_out = 1; return true;
        case ADRP_MATHV_FASIN:
        case ADRP_MATHV_FEXP:
        case ADRP_MATHV_QUAT_INV_NORM: *k_in = 1; *k_out = 1; return true;
        case ADRP_MATHV_SMALL_SINCOS:
        case ADRP_MATHV_EXPMAP_SINC_COS: *k_in = 1; *k_out = 2; return true;
        case ADRP_MATHV_CLAMP100_WV: *k_in = 6; *k_out = 6; return true;
        default: return false;
    }
}
}  // namespace

extern "C" int adrp_math_probe_v_planes(int fn, int* k_in, int* k_out) {
    int a = 0, b = 0;
    if (!mathv_planes(fn, &a, &b)) return ADRP_ERR_INVALID;
    if (k_in) *k_in = a;
    if (k_out) *k_out = b;
    return ADRP_OK;
}

extern "C" int adrp_math_probe_v(int fn, int precision, const double* in_dev, double* out_dev, int n, void* stream) {
    int k_in, k_out;
    if (!mathv_planes(fn, &k_in, &k_out) || (precision != 0 && precision != 1) || n < 0 ||
        (n > 0 && (!in_dev || !out_dev)))
        return ADRP_ERR_INVALID;
    if (n == 0) return ADRP_OK;
    if (precision == 1)
        hipLaunchKernelGGL(math_probe_v_kernel<double>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, fn, in_dev,
                           out_dev, n);
    else
        hipLaunchKernelGGL(math_probe_v_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, fn, in_dev,
                           out_dev, n);
    return hipGetLastError() == hipSuccess ? ADRP_OK : ADRP_ERR_DEVICE;
}

extern "C" int adrp_math_probe(int fn, const double* in_dev, double* out_dev, int n, void* stream) {
    if (fn < ADRP_MATH_RCP || fn > ADRP_MATH_FDIV_RCP || n < 0 || (n > 0 && (!in_dev || !out_dev))) return ADRP_ERR_INVALID;
    if (n == 0) return ADRP_OK;
    hipLaunchKernelGGL(math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, fn, in_dev, out_dev, n);
    return hipGetLastError() == hipSuccess ? ADRP_OK : ADRP_ERR_DEVICE;
}
