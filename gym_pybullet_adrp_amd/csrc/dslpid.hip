// dslpid.hip — the stand-alone batched DSLPIDControl: kernel instantiations (dslpid_kernel.h) and the
// adrp_dslpid_* C-ABI (include/adrp.h).
#include "adrp_internal.h"
#include "dslpid_kernel.h"

struct adrp_dslpid {
    int rows = 0, precision = 0, device = 0;
    void* st = nullptr;            // Real [9][rows]
    adrp_dslpid_params p;
};

static int dsl_err(int code, const std::string& msg) { return seterr(nullptr, code, msg); }

#define DSLCHK(x)                                                                               \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return dsl_err(ADRP_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

extern "C" int adrp_dslpid_default_params(int model, adrp_dslpid_params* p) {
    if (!p) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_default_params: NULL argument");
    if (model != ADRP_DSLPID_CF2X && model != ADRP_DSLPID_CF2P)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_default_params: model must be CF2X (0) or CF2P (1)");
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof(adrp_dslpid_params);
    const double pf[3] = {.4, .4, 1.25}, i_f[3] = {.05, .05, .05}, df[3] = {.2, .2, .5};
    const double pt[3] = {70000., 70000., 60000.}, it[3] = {.0, .0, 500.}, dt[3] = {20000., 20000., 12000.};
    static const double mx[4][3] = {{-.5, -.5, -1}, {-.5, .5, 1}, {.5, .5, -1}, {.5, -.5, 1}};
    static const double mp[4][3] = {{0, -1, -1}, {1, 0, 1}, {0, 1, -1}, {-1, 0, 1}};
    for (int k = 0; k < 3; ++k) {
        p->p_for[k] = pf[k]; p->i_for[k] = i_f[k]; p->d_for[k] = df[k];
        p->p_tor[k] = pt[k]; p->i_tor[k] = it[k]; p->d_tor[k] = dt[k];
    }
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k) p->mixer[i][k] = model == ADRP_DSLPID_CF2X ? mx[i][k] : mp[i][k];
    p->gravity = 9.8 * (model == ADRP_DSLPID_CF2X ? 0.03454 : 0.027);
    p->kf = 3.16e-10;
    p->pwm2rpm_scale = 0.2685; p->pwm2rpm_const = 4070.3;
    p->min_pwm = 20000; p->max_pwm = 65535;
    return ADRP_OK;
}

extern "C" int adrp_dslpid_create(int rows, int precision, const adrp_dslpid_params* p, int device, adrp_dslpid_t** out) {
    if (!out) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_create: out is NULL");
    *out = nullptr;
    if (rows <= 0) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_create: rows must be > 0");
    if (precision != 0 && precision != 1) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_create: precision must be 0 or 1");
    if (!p || p->struct_size != sizeof(adrp_dslpid_params))
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_create: adrp_dslpid_params.struct_size mismatch (ABI)");
    if (!(p->kf > 0) || !(p->pwm2rpm_scale > 0))
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_create: kf and pwm2rpm_scale must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return dsl_err(ADRP_ERR_DEVICE, "no HIP device visible (libadrp has no CPU fallback)");
    if (device < 0 || device >= ndev) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_create: device index out of range");
    adrp_dslpid_t* c = new adrp_dslpid_t();
    c->rows = rows; c->precision = precision; c->device = device; c->p = *p;
    DeviceGuard g(device);
    const size_t bytes = size_t(kDslpidState) * rows * (precision ? 8 : 4);
    if (hipMalloc(&c->st, bytes) != hipSuccess) {
        delete c;
        return dsl_err(ADRP_ERR_OOM, "adrp_dslpid_create: hipMalloc failed");
    }
    if (hipMemset(c->st, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        hipFree(c->st);
        delete c;
        return dsl_err(ADRP_ERR_DEVICE, "adrp_dslpid_create: initialisation failed");
    }
    *out = c;
    return ADRP_OK;
}

extern "C" void adrp_dslpid_destroy(adrp_dslpid_t* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    hipDeviceSynchronize();
    hipFree(c->st);
    delete c;
}

extern "C" int adrp_dslpid_reset(adrp_dslpid_t* c, const uint8_t* mask_dev, void* stream) {
    if (!c) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_reset: NULL argument");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (!mask_dev) {
        DSLCHK(hipMemsetAsync(c->st, 0, size_t(kDslpidState) * c->rows * (c->precision ? 8 : 4), s));
        return ADRP_OK;
    }
    const dim3 grid((unsigned)((c->rows + 255) / 256)), blk(256);
    if (c->precision) hipLaunchKernelGGL(dslpid_reset_kernel<double>, grid, blk, 0, s, (double*)c->st, mask_dev, c->rows);
    else hipLaunchKernelGGL(dslpid_reset_kernel<float>, grid, blk, 0, s, (float*)c->st, mask_dev, c->rows);
    DSLCHK(hipGetLastError());
    return ADRP_OK;
}

extern "C" int adrp_dslpid_set_gains(adrp_dslpid_t* c, const adrp_dslpid_params* p) {
    if (!c) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_set_gains: NULL argument");
    if (!p || p->struct_size != sizeof(adrp_dslpid_params))
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_set_gains: adrp_dslpid_params.struct_size mismatch (ABI)");
    for (int k = 0; k < 3; ++k) {
        c->p.p_for[k] = p->p_for[k]; c->p.i_for[k] = p->i_for[k]; c->p.d_for[k] = p->d_for[k];
        c->p.p_tor[k] = p->p_tor[k]; c->p.i_tor[k] = p->i_tor[k]; c->p.d_tor[k] = p->d_tor[k];
    }
    return ADRP_OK;
}

extern "C" int adrp_dslpid_get_state(adrp_dslpid_t* c, void* st_dev, void* stream) {
    if (!c || !st_dev) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_get_state: NULL argument");
    DeviceGuard g(c->device);
    DSLCHK(hipMemcpyAsync(st_dev, c->st, size_t(kDslpidState) * c->rows * (c->precision ? 8 : 4), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return ADRP_OK;
}

extern "C" int adrp_dslpid_set_state(adrp_dslpid_t* c, const void* st_dev, void* stream) {
    if (!c || !st_dev) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_set_state: NULL argument");
    DeviceGuard g(c->device);
    DSLCHK(hipMemcpyAsync(c->st, st_dev, size_t(kDslpidState) * c->rows * (c->precision ? 8 : 4), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return ADRP_OK;
}

template <typename Real>
static DslpidConst<Real> dslpid_const(const adrp_dslpid_params& p, double dt) {
    DslpidConst<Real> k;
    for (int j = 0; j < 3; ++j) {
        k.p_for[j] = Real(p.p_for[j]); k.i_for[j] = Real(p.i_for[j]); k.d_for[j] = Real(p.d_for[j]);
        k.p_tor[j] = Real(p.p_tor[j]); k.i_tor[j] = Real(p.i_tor[j]); k.d_tor[j] = Real(p.d_tor[j]);
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) k.mix[i][j] = Real(p.mixer[i][j]);
    k.grav = Real(p.gravity); k.inv4kf = Real(1.0 / (4.0 * p.kf));
    k.rpm_scale = Real(p.pwm2rpm_scale); k.rpm_const = Real(p.pwm2rpm_const); k.inv_scale = Real(1.0 / p.pwm2rpm_scale);
    k.min_pwm = Real(p.min_pwm); k.max_pwm = Real(p.max_pwm);
    k.dt = Real(dt); k.hz = Real(1.0 / dt);
    return k;
}

struct DslpidIo {
    const void *pos, *quat, *vel;
    long long cs[3], rs[3];      // component / row strides of pos, quat, vel (elements)
    const void *t_pos, *t_rpy, *t_vel, *t_rates;
    void *rpm, *pos_e, *yaw_e;
};

template <typename Real, typename TIn>
static int dslpid_launch(adrp_dslpid_t* c, double dt, const DslpidIo& io, hipStream_t s) {
    DslpidArgs<Real, TIn> a;
    a.k = dslpid_const<Real>(c->p, dt);
    a.pos = {(const TIn*)io.pos, io.cs[0], io.rs[0]};
    a.quat = {(const TIn*)io.quat, io.cs[1], io.rs[1]};
    a.vel = {(const TIn*)io.vel, io.cs[2], io.rs[2]};
    a.t_pos = (const Real*)io.t_pos; a.t_rpy = (const Real*)io.t_rpy;
    a.t_vel = (const Real*)io.t_vel; a.t_rates = (const Real*)io.t_rates;
    a.st = (Real*)c->st;
    a.rpm = (Real*)io.rpm; a.pos_e = (Real*)io.pos_e; a.yaw_e = (Real*)io.yaw_e;
    a.rows = c->rows;
    const dim3 grid((unsigned)((c->rows + kDslpidBlock - 1) / kDslpidBlock)), blk(kDslpidBlock);
    hipLaunchKernelGGL((dslpid_control_kernel<Real, TIn>), grid, blk, 0, s, a);
    DSLCHK(hipGetLastError());
    return ADRP_OK;
}

static int dslpid_dispatch(adrp_dslpid_t* c, double dt, int input_precision, const DslpidIo& io, hipStream_t s) {
    DeviceGuard g(c->device);
    if (!c->precision) return dslpid_launch<float, float>(c, dt, io, s);
    return input_precision ? dslpid_launch<double, double>(c, dt, io, s) : dslpid_launch<double, float>(c, dt, io, s);
}

extern "C" int adrp_dslpid_compute(adrp_dslpid_t* c, double control_timestep, const void* pos_dev, const void* quat_dev,
                                   const void* vel_dev, int row_stride, int input_precision, const void* target_pos_dev,
                                   const void* target_rpy_dev, const void* target_vel_dev,
                                   const void* target_rpy_rates_dev, void* rpm_out, void* pos_e_out, void* yaw_e_out,
                                   void* stream) {
    // (the scalar first: the refusal reads the same with no controller at hand, i.e. on a machine without a GPU)
    if (!(control_timestep > 0)) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute: control_timestep must be > 0");
    if (!c || !pos_dev || !quat_dev || !vel_dev || !rpm_out)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute: NULL argument");
    if (row_stride < 0) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute: row_stride must be >= 0");
    if (input_precision != 0 && input_precision != 1)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute: input_precision must be 0 or 1");
    if (input_precision == 1 && c->precision == 0)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute: float64 inputs need a float64 controller");
    DslpidIo io;
    io.pos = pos_dev; io.quat = quat_dev; io.vel = vel_dev;
    io.cs[0] = io.cs[1] = io.cs[2] = 1;
    io.rs[0] = row_stride ? row_stride : 3; io.rs[1] = row_stride ? row_stride : 4; io.rs[2] = row_stride ? row_stride : 3;
    io.t_pos = target_pos_dev; io.t_rpy = target_rpy_dev; io.t_vel = target_vel_dev; io.t_rates = target_rpy_rates_dev;
    io.rpm = rpm_out; io.pos_e = pos_e_out; io.yaw_e = yaw_e_out;
    return dslpid_dispatch(c, control_timestep, input_precision, io, (hipStream_t)stream);
}

extern "C" int adrp_dslpid_compute_env(adrp_dslpid_t* c, double control_timestep, adrp_t* h, const void* target_pos_dev,
                                       const void* target_rpy_dev, const void* target_vel_dev,
                                       const void* target_rpy_rates_dev, void* rpm_out, void* pos_e_out, void* yaw_e_out,
                                       void* stream) {
    if (!(control_timestep > 0)) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: control_timestep must be > 0");
    if (!c || !h || !rpm_out) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: NULL argument");
    if (h->cfg.task == ADRP_TASK_RACE)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: MultiRaceAviary handles are not supported");
    if ((long long)h->E * h->N != c->rows)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: the handle's E * N differs from the controller's rows");
    if (int(h->real_size == 8) != c->precision)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: the handle's precision differs from the controller's");
    if (h->device != c->device)
        return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: the handle lives on another device");
    if (h->pbox) return dsl_err(ADRP_ERR_INVALID, "adrp_dslpid_compute_env: persistent mode is active (adrp_persistent_end first)");
    // state snapshot columns: field k of column r at f[k * EN + r] (HoverField)
    const long long EN = c->rows;
    const size_t rb = h->real_size;
    DslpidIo io;
    io.pos = (const char*)h->f + size_t(HF_POS) * EN * rb;
    io.quat = (const char*)h->f + size_t(HF_QUAT) * EN * rb;
    io.vel = (const char*)h->f + size_t(HF_VEL) * EN * rb;
    io.cs[0] = io.cs[1] = io.cs[2] = EN;
    io.rs[0] = io.rs[1] = io.rs[2] = 1;
    io.t_pos = target_pos_dev; io.t_rpy = target_rpy_dev; io.t_vel = target_vel_dev; io.t_rates = target_rpy_rates_dev;
    io.rpm = rpm_out; io.pos_e = pos_e_out; io.yaw_e = yaw_e_out;
    return dslpid_dispatch(c, control_timestep, c->precision, io, (hipStream_t)stream);
}
