// mellinger.hip — the stand-alone batched MellingerControl: kernel instantiations (mellinger_kernel.h) and
// the adrp_mellinger_* C-ABI (include/adrp.h).  Compiled with the race translation units' flags, so the
// controller functions it shares with them round as they do there.
#include "adrp_internal.h"
#include "mellinger_kernel.h"

struct adrp_mellinger {
    int rows = 0, precision = 0, device = 0;
    void* st = nullptr;            // Real [MF_N][rows]
    int32_t* ist = nullptr;        // [MI_N][rows]
    float* cf = nullptr;           // [ADRP_CMD_NF][rows]
    int32_t* ci = nullptr;         // [ADRP_CMD_NI][rows]
    uint32_t* ticks = nullptr;     // race_tick_tables
    Lpf lpf;
};

static int mel_err(int code, const std::string& msg) { return seterr(nullptr, code, msg); }

#define MELCHK(x)                                                                               \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return mel_err(ADRP_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

static const char* k_mell_f[MF_N] = {
    "rpm_0", "rpm_1", "rpm_2", "rpm_3", "prev_rpm_0", "prev_rpm_1", "prev_rpm_2", "prev_rpm_3",
    "prev_rpy_0", "prev_rpy_1", "prev_rpy_2", "prev_vel_0", "prev_vel_1", "prev_vel_2",
    "lpf_d1_0", "lpf_d1_1", "lpf_d1_2", "lpf_d2_0", "lpf_d2_1", "lpf_d2_2",
    "i_err_0", "i_err_1", "i_err_2", "i_err_m_0", "i_err_m_1", "i_err_m_2",
    "prev_omega_roll", "prev_omega_pitch", "prev_sp_roll", "prev_sp_pitch",
    "ctl_roll", "ctl_pitch", "ctl_yaw", "ctl_thrust"};
static const char* k_mell_i[MI_N] = {"tick", "last_att_tick", "last_pos_tick", "tumble"};

static size_t mel_real(const adrp_mellinger_t* c) { return c->precision ? 8 : 4; }

static void mel_free(adrp_mellinger_t* c) {
    hipFree(c->st); hipFree(c->ist); hipFree(c->cf); hipFree(c->ci); hipFree(c->ticks);
    delete c;
}

template <typename Real, typename TIn>
static MellArgs<Real, TIn> mel_args(const adrp_mellinger_t* c) {
    MellArgs<Real, TIn> a;
    memset(&a, 0, sizeof a);
    a.st = (Real*)c->st; a.ist = c->ist; a.cf = c->cf; a.ci = c->ci; a.ticks = c->ticks;
    a.lpf = c->lpf;
    a.rows = c->rows;
    return a;
}

static dim3 mel_grid(const adrp_mellinger_t* c) { return dim3((unsigned)((c->rows + kMellBlock - 1) / kMellBlock)); }

struct MellIo {
    const void *pos, *ang, *vel;
    long long cs[3], rs[3];      // component / row strides of pos, ang, vel (elements)
    const void *noise, *mask;
    void *rpm, *rpy_out;
};

template <typename Real, typename TIn>
static MellArgs<Real, TIn> mel_io_args(const adrp_mellinger_t* c, const MellIo& io) {
    MellArgs<Real, TIn> a = mel_args<Real, TIn>(c);
    a.pos = {(const TIn*)io.pos, io.cs[0], io.rs[0]};
    a.ang = {(const TIn*)io.ang, io.cs[1], io.rs[1]};
    a.vel = {(const TIn*)io.vel, io.cs[2], io.rs[2]};
    a.noise = (const Real*)io.noise;
    a.mask = (const uint8_t*)io.mask;
    a.rpm = (Real*)io.rpm;
    a.rpy_out = (Real*)io.rpy_out;
    return a;
}

template <typename Real, typename TIn, bool ENV>
static int mel_launch(adrp_mellinger_t* c, const MellIo& io, hipStream_t s) {
    const MellArgs<Real, TIn> a = mel_io_args<Real, TIn>(c, io);
    hipLaunchKernelGGL((mellinger_compute_kernel<Real, TIn, ENV>), mel_grid(c), dim3(kMellBlock), 0, s, a);
    MELCHK(hipGetLastError());
    return ADRP_OK;
}

extern "C" int adrp_mellinger_create(int rows, int precision, int device, adrp_mellinger_t** out) {
    if (!out) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_create: out is NULL");
    *out = nullptr;
    if (rows <= 0) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_create: rows must be > 0");
    if (precision != 0 && precision != 1) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_create: precision must be 0 or 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return mel_err(ADRP_ERR_DEVICE, "no HIP device visible (libadrp has no CPU fallback)");
    if (device < 0 || device >= ndev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_create: device index out of range");
    adrp_mellinger_t* c = new adrp_mellinger_t();
    c->rows = rows; c->precision = precision; c->device = device;
    float l[5];
    race_gyro_lpf(l);
    c->lpf = {l[0], l[1], l[2], l[3], l[4]};
    DeviceGuard g(device);
    const size_t n = size_t(rows);
    std::vector<uint32_t> ticks(2 * kTickWords);
    race_tick_tables(ticks.data(), ticks.data() + kTickWords);
    if (hipMalloc(&c->st, MF_N * n * mel_real(c)) != hipSuccess || hipMalloc(&c->ist, MI_N * n * 4) != hipSuccess ||
        hipMalloc(&c->cf, ADRP_CMD_NF * n * 4) != hipSuccess || hipMalloc(&c->ci, ADRP_CMD_NI * n * 4) != hipSuccess ||
        hipMalloc(&c->ticks, ticks.size() * 4) != hipSuccess) {
        mel_free(c);
        return mel_err(ADRP_ERR_OOM, "adrp_mellinger_create: hipMalloc failed");
    }
    // every row as reset() at the origin leaves it
    bool ok = hipMemcpy(c->ticks, ticks.data(), ticks.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(c->st, 0, MF_N * n * mel_real(c)) == hipSuccess;
    if (ok) {
        MellIo io = {};
        io.pos = io.ang = io.vel = c->st;   // (zeros)
        io.cs[0] = io.cs[1] = io.cs[2] = 1;
        io.rs[0] = io.rs[1] = io.rs[2] = 0;
        if (precision) {
            const MellArgs<double, double> a = mel_io_args<double, double>(c, io);
            hipLaunchKernelGGL((mellinger_reset_kernel<double, double>), mel_grid(c), dim3(kMellBlock), 0, 0, a);
        } else {
            const MellArgs<float, float> a = mel_io_args<float, float>(c, io);
            hipLaunchKernelGGL((mellinger_reset_kernel<float, float>), mel_grid(c), dim3(kMellBlock), 0, 0, a);
        }
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) {
        mel_free(c);
        return mel_err(ADRP_ERR_DEVICE, "adrp_mellinger_create: initialisation failed");
    }
    *out = c;
    return ADRP_OK;
}

extern "C" void adrp_mellinger_destroy(adrp_mellinger_t* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    hipDeviceSynchronize();
    mel_free(c);
}

extern "C" int adrp_mellinger_reset(adrp_mellinger_t* c, const void* pos_dev, const void* rpy_dev, const void* vel_dev,
                                    const uint8_t* mask_dev, void* stream) {
    if (!c || !pos_dev || !rpy_dev || !vel_dev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_reset: NULL argument");
    DeviceGuard g(c->device);
    MellIo io = {};
    io.pos = pos_dev; io.ang = rpy_dev; io.vel = vel_dev;
    io.cs[0] = io.cs[1] = io.cs[2] = 1;
    io.rs[0] = io.rs[1] = io.rs[2] = 3;
    io.mask = mask_dev;
    if (c->precision) {
        const MellArgs<double, double> a = mel_io_args<double, double>(c, io);
        hipLaunchKernelGGL((mellinger_reset_kernel<double, double>), mel_grid(c), dim3(kMellBlock), 0, (hipStream_t)stream, a);
    } else {
        const MellArgs<float, float> a = mel_io_args<float, float>(c, io);
        hipLaunchKernelGGL((mellinger_reset_kernel<float, float>), mel_grid(c), dim3(kMellBlock), 0, (hipStream_t)stream, a);
    }
    MELCHK(hipGetLastError());
    return ADRP_OK;
}

extern "C" int adrp_mellinger_command(adrp_mellinger_t* c, const int32_t* codes_dev, const double* args_dev, void* stream) {
    if (!c || !codes_dev || !args_dev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_command: NULL argument");
    DeviceGuard g(c->device);
    MellArgs<float, float> a = mel_args<float, float>(c);   // (the command state is float at every precision)
    a.st = nullptr;
    a.cmd = codes_dev; a.cargs = args_dev;
    hipLaunchKernelGGL((mellinger_command_kernel<float, float>), mel_grid(c), dim3(kMellBlock), 0, (hipStream_t)stream, a);
    MELCHK(hipGetLastError());
    return ADRP_OK;
}

extern "C" int adrp_mellinger_compute(adrp_mellinger_t* c, const void* pos_dev, const void* rpy_dev, const void* vel_dev,
                                      int row_stride, int input_precision, const void* disturbance_dev, void* rpm_out,
                                      void* stream) {
    if (!c || !pos_dev || !rpy_dev || !vel_dev || !rpm_out)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute: NULL argument");
    if (row_stride < 0) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute: row_stride must be >= 0");
    if (input_precision != 0 && input_precision != 1)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute: input_precision must be 0 or 1");
    if (input_precision == 1 && c->precision == 0)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute: float64 inputs need a float64 controller");
    MellIo io = {};
    io.pos = pos_dev; io.ang = rpy_dev; io.vel = vel_dev;
    io.cs[0] = io.cs[1] = io.cs[2] = 1;
    io.rs[0] = io.rs[1] = io.rs[2] = row_stride ? row_stride : 3;
    io.noise = disturbance_dev; io.rpm = rpm_out;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (!c->precision) return mel_launch<float, float, false>(c, io, s);
    return input_precision ? mel_launch<double, double, false>(c, io, s) : mel_launch<double, float, false>(c, io, s);
}

extern "C" int adrp_mellinger_compute_env(adrp_mellinger_t* c, adrp_t* h, const void* disturbance_dev, void* rpm_out,
                                          void* rpy_out, void* stream) {
    if (!c || !h || !rpm_out) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute_env: NULL argument");
    if (h->cfg.task != ADRP_TASK_CTRL)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute_env: only CtrlAviary handles are supported");
    if ((long long)h->E * h->N != c->rows)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute_env: the handle's E * N differs from the controller's rows");
    if (int(h->real_size == 8) != c->precision)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute_env: the handle's precision differs from the controller's");
    if (h->device != c->device)
        return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute_env: the handle lives on another device");
    if (h->pbox) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_compute_env: persistent mode is active (adrp_persistent_end first)");
    // state snapshot columns: field k of column r at f[k * EN + r] (HoverField)
    const long long EN = c->rows;
    const size_t rb = h->real_size;
    MellIo io = {};
    io.pos = (const char*)h->f + size_t(HF_POS) * EN * rb;
    io.ang = (const char*)h->f + size_t(HF_QUAT) * EN * rb;
    io.vel = (const char*)h->f + size_t(HF_VEL) * EN * rb;
    io.cs[0] = io.cs[1] = io.cs[2] = EN;
    io.rs[0] = io.rs[1] = io.rs[2] = 1;
    io.noise = disturbance_dev; io.rpm = rpm_out; io.rpy_out = rpy_out;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    return c->precision ? mel_launch<double, double, true>(c, io, s) : mel_launch<float, float, true>(c, io, s);
}

extern "C" int adrp_mellinger_state_layout(const adrp_mellinger_t*, int* nf, int* ni) {
    if (!nf || !ni) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_state_layout: NULL argument");
    *nf = MF_N; *ni = MI_N;
    return ADRP_OK;
}

extern "C" const char* adrp_mellinger_state_field(int is_int, int index) {
    if (index < 0 || index >= (is_int ? int(MI_N) : int(MF_N))) return nullptr;
    return is_int ? k_mell_i[index] : k_mell_f[index];
}

extern "C" int adrp_mellinger_get_state(adrp_mellinger_t* c, void* f_dev, int32_t* i_dev, void* stream) {
    if (!c || !f_dev || !i_dev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_get_state: NULL argument");
    DeviceGuard g(c->device);
    const size_t n = size_t(c->rows);
    MELCHK(hipMemcpyAsync(f_dev, c->st, MF_N * n * mel_real(c), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    MELCHK(hipMemcpyAsync(i_dev, c->ist, MI_N * n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADRP_OK;
}

extern "C" int adrp_mellinger_set_state(adrp_mellinger_t* c, const void* f_dev, const int32_t* i_dev, void* stream) {
    if (!c || !f_dev || !i_dev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_set_state: NULL argument");
    DeviceGuard g(c->device);
    const size_t n = size_t(c->rows);
    MELCHK(hipMemcpyAsync(c->st, f_dev, MF_N * n * mel_real(c), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    MELCHK(hipMemcpyAsync(c->ist, i_dev, MI_N * n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADRP_OK;
}

extern "C" int adrp_mellinger_get_command_state(adrp_mellinger_t* c, float* f_dev, int32_t* i_dev, void* stream) {
    if (!c || !f_dev || !i_dev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_get_command_state: NULL argument");
    DeviceGuard g(c->device);
    const size_t n = size_t(c->rows);
    MELCHK(hipMemcpyAsync(f_dev, c->cf, ADRP_CMD_NF * n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    MELCHK(hipMemcpyAsync(i_dev, c->ci, ADRP_CMD_NI * n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADRP_OK;
}

extern "C" int adrp_mellinger_set_command_state(adrp_mellinger_t* c, const float* f_dev, const int32_t* i_dev, void* stream) {
    if (!c || !f_dev || !i_dev) return mel_err(ADRP_ERR_INVALID, "adrp_mellinger_set_command_state: NULL argument");
    DeviceGuard g(c->device);
    const size_t n = size_t(c->rows);
    MELCHK(hipMemcpyAsync(c->cf, f_dev, ADRP_CMD_NF * n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    MELCHK(hipMemcpyAsync(c->ci, i_dev, ADRP_CMD_NI * n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ADRP_OK;
}
