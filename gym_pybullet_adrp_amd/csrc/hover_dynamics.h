// hover_dynamics.h — what the hover, multi-hover, ctrl and persistent step kernels share: the per-config
// constants, one drone's state (Body) and what the sub-step chain carries (Chain), the Bullet sub-step
// (pyb_substep, its translational half pyb_trans_*) and the explicit model (dyn_substep), the reset draw,
// the obs row, the state's field loads and stores, and the sub-step chain of one env.step (pyb_chain).
// The reference lines are listed at the head of hover_kernel.h.
//
// Closed form used per Bullet sub-step (derivation in DESIGN.md §Kernel):
//   thrust axis  zs = Rs·ẑ  (Rs = link basis cached at the last forwardKinematics)
//   F_world      = Σf·zs + [Σg·R·ẑ] + B·f_link4 + m·g
//   n_body       = P × (Rᵀzs) + τz·(Rᵀzs) + [G × ẑ]          P = Σ f_i p_i, G = Σ g_i p_i
//   ω̇_b          = I⁻¹(n_b − k(1+|ω_b|) I∘ω_b − ω_b × I ω_b),   a_w = F_w/m − k(1+|v|) v
//   v, ω += dt(·) (clamped ±100);  x += dt v;  q ← normalize((ω̂ sin, cos) ⊗ q)
// ω is carried in the BODY frame through the sub-steps (wb = Rᵀω; state, obs and Bullet's API keep
// the world frame: one rotation in before the loop, one out after it).  The exp map rotates the pose
// about ω' itself, R' = exp([ω' dt]) R, so R'ᵀω' = Rᵀω' and
//   wb' = wb + dt I⁻¹(n_b − k(1+|wb|) I∘wb − wb × I wb)          exactly, no rotation either way
//   q'  = normalize(q ⊗ (s·wb', c))                              s = sin(|wb'|dt/2)/|wb'|, c = cos
//   R'ᵀ col2(R) = third row of rot(δ), δ = (s·wb', c)/|q₁|       the next sub-step's Rᵀzs (lag on)
//               = (2(δxδz − δwδy), 2(δyδz + δwδx), 1 − 2(δx² + δy²))
// so no sub-step multiplies by a rotation matrix.  Per physics mode (template, no runtime branch):
//   PYB, PYB_DW            third columns only: zs (lagged, thrust), zc (current, contact test)
//   PYB_GND, .._GND_DRAG_DW  additionally the third row of the current R (prop heights) and zc
//   PYB_DRAG               whole R and lagged Rs for Rs (Rᵀ drag): carries both matrices
//   DYN                    its own explicit model (dyn_substep)
// The ±100 clamp is on WORLD coordinates of ω: none can exceed 100 unless |wb| does, so behind a
// wave-uniform __any(|wb| > 100): w = R wb, clamp, wb = Rᵀ w, committed per lane only where the
// lane's own |wb| > 100 (clamp100_body; batch invariance).
#pragma once

#include "adrp_device.h"
#include "dslpid_core.h"

namespace adrp {

// float-field indices of the HoverAviary state snapshot ([field][E], SoA)
enum HoverField {
    HF_POS = 0, HF_QUAT = 3, HF_VEL = 7, HF_OMEGA = 10, HF_LAST_RPM = 13, HF_ANGV = 17,
    HF_LINK_QUAT = 20, HF_NBASE = 24,
    // DSLPIDControl state (PID / VEL / ONE_D_PID handles only): last_rpy 3, integral_pos_e 3,
    // integral_rpy_e 3 (control/DSLPIDControl.py:65-79)
    HF_PID = 24, HF_NPID = 9
};
enum HoverInt { HI_STEP = 0, HI_EPISODE = 1, HI_RING_HEAD = 2, HI_N = 3 };

// Per-config constants.  Device-resident (one block per handle, written at create, warm
// in L2 across launches), or compiled in as literals for the reference's default drone
// (cf2x_consts: CF2X / cf2x_IROS.urdf at 240 Hz), where they fold into immediates.
template <typename Real>
struct HoverConst {
    int S, trunc_steps, link_lag, physics;   // truncated once step_counter >= trunc_steps
    Real dt, mass, inv_mass, gravity;
    Real ixx, iyy, izz, inv_ixx, inv_iyy, inv_izz;
    Real kf, km, hover_rpm;
    Real px[4], py[4], pz[4];                // prop link COM offsets (body)
    Real gnd_kf, prop_r4, gnd_clip;          // kf*GND_EFF_COEFF, PROP_RADIUS/4, GND_EFF_H_CLIP
    Real drag[3];
    Real dyn_arm;                            // L/sqrt(2) (Physics.DYN)
    Real coll_hh, coll_r, coll_zoff;         // collision cylinder half-height, radius, z offset
    Real ang_max;                            // ANGULAR_MOTION_THRESHOLD / dt
    Real target[3];
    // DSLPIDControl (PID / VEL / ONE_D_PID): GRAVITY = g*m (BaseControl.py:35, the env's own
    // URDF), 1/(4 KF), CTRL_TIMESTEP and its inverse, SPEED_LIMIT as the float32 NumPy uses
    Real pid_grav, pid_inv4kf, ctrl_dt, ctrl_hz;
    float speed_limit;
};

// HoverAviary defaults: cf2x_IROS.urdf, PYB_FREQ 240, CTRL_FREQ 30, target (0,0,1), 8 s.
// Derived values are the float64 results of BaseAviary.py:117-128's formulas; the host
// selects this path only when its computed block is bit-identical (adrp.hip).
template <typename Real>
__host__ __device__ constexpr HoverConst<Real> cf2x_consts(int physics) {
    HoverConst<Real> c{};
    c.S = 8; c.trunc_steps = 1921; c.link_lag = 1; c.physics = physics;
    c.dt = Real(0.004166666666666667);
    c.mass = Real(0.03454); c.inv_mass = Real(28.951939779965258); c.gravity = Real(9.8);
    c.ixx = Real(1.4e-5); c.iyy = Real(1.4e-5); c.izz = Real(2.17e-5);
    c.inv_ixx = Real(71428.57142857143); c.inv_iyy = Real(71428.57142857143); c.inv_izz = Real(46082.949308755764);
    c.kf = Real(3.16e-10); c.km = Real(7.94e-12); c.hover_rpm = Real(16364.421890108686);
    c.px[0] = Real(0.028); c.px[1] = Real(-0.028); c.px[2] = Real(-0.028); c.px[3] = Real(0.028);
    c.py[0] = Real(0.028); c.py[1] = Real(0.028); c.py[2] = Real(-0.028); c.py[3] = Real(-0.028);
    c.pz[0] = Real(0); c.pz[1] = Real(0); c.pz[2] = Real(0); c.pz[3] = Real(0);
    c.gnd_kf = Real(3.5924744399999996e-09); c.prop_r4 = Real(0.0057837); c.gnd_clip = Real(0.03776371349209501);
    c.drag[0] = Real(9.1785e-7); c.drag[1] = Real(9.1785e-7); c.drag[2] = Real(10.311e-7);
    c.dyn_arm = Real(0.028072139213105935);
    c.coll_hh = Real(0.0125); c.coll_r = Real(0.06); c.coll_zoff = Real(0);
    c.ang_max = Real(188.49555921538757);
    c.target[0] = Real(0); c.target[1] = Real(0); c.target[2] = Real(1);
    c.pid_grav = Real(0.338492); c.pid_inv4kf = Real(791139240.5063292);
    c.ctrl_dt = Real(0.03333333333333333); c.ctrl_hz = Real(30);
    c.speed_limit = 0.25f;
    return c;
}

// reset distribution (only the auto-reset / reset path reads it)
template <typename Real>
struct HoverReset {
    Real init_xyz[3], init_rpy[3], n_xyz[3], n_rpy[3], n_vel[3], n_om[3];
};

// kernel argument block: pointers and a few scalars only (it is rewritten for every
// launch, so it is cold in every cache: keep it to two 64-byte lines)
constexpr int kStepBlock = 64;   // envs per workgroup: one chain wave (E = 4096 -> 64 CUs)

template <typename Real>
struct HoverArgs {
    const HoverConst<Real>* c;   // device-resident constants (generic path)
    const HoverReset<Real>* r;
    Real* f;           // [HF_NBASE][E]
    float* ring;       // [B][E][A]  (slot-major, the A floats of one env contiguous)
    int32_t* ist;      // [HI_N][E]
    const float* act;  // [E][A]
    float* obs;        // [E][D]
    float* rew;
    uint8_t* term;
    uint8_t* trunc;
    float* tobs;       // [E][D] or null
    const uint8_t* mask;  // reset mask or null
    int32_t* contact_count;  // device counter of ground-model hits (diagnostics) or null
    uint64_t seed;
    int64_t env_offset;
    int E, B, D, autoreset;
};

template <typename Real>
struct Body {
    V3<Real> pos, vel, w;     // w: world ω (PYB) or body rpy_rates (DYN)
    Q4<Real> q, ql;           // pose quaternion, cached link basis
    V3<Real> angv;            // DYN: world ω reported by getBaseVelocity
    Real prev_rpm[4];
};

// Explicit fused multiply-adds of the PYB sub-step chain.  The hover TUs contract a*b+c only
// within one source expression (csrc/Makefile CONTRACT: the same bits in every dispatch variant),
// so the fusions across the V3 operators that the chain wants are written out here.
__device__ __forceinline__ float fmx(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmx(double a, double b, double c) { return __builtin_fma(a, b, c); }

// rot(q) with its products folded into FMAs (20 operations instead of 24)
template <typename Real>
__device__ __forceinline__ M3<Real> rot_fm(Q4<Real> q) {
    const Real x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const Real xx = q.x * x2, zz = q.z * z2;
    const Real wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
    return {Real(1) - fmx(q.y, y2, zz), fmx(q.x, y2, -wz), fmx(q.x, z2, wy),
            fmx(q.x, y2, wz), Real(1) - fmx(q.x, x2, zz), fmx(q.y, z2, -wx),
            fmx(q.x, z2, -wy), fmx(q.y, z2, wx), Real(1) - fmx(q.y, y2, xx)};
}

// float32 1 + 0.05 a, two roundings as NumPy does it (no FMA contraction)
__device__ __forceinline__ float rpm_gain(float a) {
#pragma clang fp contract(off)
    const float m = 0.05f * a;
    return 1.0f + m;
}

// third column (body z axis in world) and third row of rot_fm(q): the same expressions, so the same bits
template <typename Real>
__device__ __forceinline__ V3<Real> col2_fm(Q4<Real> q) {
    const Real x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const Real xx = q.x * x2;
    const Real wx = q.w * x2, wy = q.w * y2;
    return {fmx(q.x, z2, wy), fmx(q.y, z2, -wx), Real(1) - fmx(q.y, y2, xx)};
}
template <typename Real>
__device__ __forceinline__ V3<Real> row2_fm(Q4<Real> q) {
    const Real x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const Real xx = q.x * x2;
    const Real wx = q.w * x2, wy = q.w * y2;
    return {fmx(q.x, z2, -wy), fmx(q.y, z2, wx), Real(1) - fmx(q.y, y2, xx)};
}

// What the PYB sub-step chain carries from one sub-step to the next beside the Body.  ω lives in the
// body frame inside the loop (header comment: no rotation of ω either way, no rotation matrix).
template <typename Real>
struct Chain {
    V3<Real> wb;      // body-frame angular velocity R^T ω
    Real wn;          // |wb| (= |ω|: the damping term's and the exp map's norm, one sqrt per sub-step)
    V3<Real> zs;      // thrust axis: third column of the cached link basis (world)
    V3<Real> zc;      // third column of the current pose's matrix (world)
    V3<Real> m3;      // R^T zs
    V3<Real> dti;     // dt I^-1
    M3<Real> R, Rs;   // PYB_DRAG only (drag goes world -> body -> cached link basis): rot_fm(q), rot_fm(ql)
};

__device__ __forceinline__ float clamp100_(float x) { return __builtin_amdgcn_fmed3f(x, -100.0f, 100.0f); }
__device__ __forceinline__ double clamp100_(double x) { return clamp100_sel(x); }

// btClamp(x, -100, 100) of the six coordinate velocities (clamp100_wv) for the body-frame chain.
// v as there.  ω's coordinates are WORLD coordinates; none can exceed 100 unless |wb| = |ω| does, so
// behind a wave-uniform test of the norm: w = R wb, clamp, wb = R^T w, and the norm again, with R the
// pre-update pose's matrix (what Bullet clamps against).  The result is committed per lane, only where
// the lane's own |wb| > 100: a slow env never takes the round trip because a wave mate spins fast
// (batch invariance).  NaN fails the test and passes through, as in btClamp.
// VEL = false: ω alone (v is not read: the translation wave clamps it, clamp100_vel)
template <typename Real, bool VEL = true>
__device__ __forceinline__ void clamp100_body(Q4<Real> q, V3<Real>& wb, Real& wn, V3<Real>& v, const ChainK<Real>& K) {
    const Real c = K.c100;
    const bool fast = wn > c;
    bool big = fast;
    if constexpr (!VEL) {
    } else if constexpr (sizeof(Real) == 8) {   // (fp64 has no med3: the select form of v's clamp goes behind the test too)
        const bool bx = fabs_(v.x) > c, by = fabs_(v.y) > c, bz = fabs_(v.z) > c;
        big = fast | bx | by | bz;
    } else {
        v = v3(clamp100_(v.x), clamp100_(v.y), clamp100_(v.z));
    }
    if (__builtin_expect(__any(big), 0)) {
        if constexpr (VEL && sizeof(Real) == 8) v = v3(clamp100_(v.x), clamp100_(v.y), clamp100_(v.z));
        const M3<Real> R = rot_fm(q);
        const V3<Real> w = mul(R, wb);
        const V3<Real> wc = mulT(R, v3(clamp100_(w.x), clamp100_(w.y), clamp100_(w.z)));
        const Real wnc = hsqrt_nn_(dot(wc, wc), K);
        wb = v3(fast ? wc.x : wb.x, fast ? wc.y : wb.y, fast ? wc.z : wb.z);
        wn = fast ? wnc : wn;
    }
}
// v's half of clamp100_body on a wave of its own.  The clamp is a select per component that leaves a
// component inside +-100 (and a NaN) as it is, so which wave mates send the wave into it changes no lane's
// value: voting on v alone here and on ω alone there gives every lane what the common vote gave it.
template <typename Real>
__device__ __forceinline__ void clamp100_vel(V3<Real>& v, const ChainK<Real>& K) {
    if constexpr (sizeof(Real) == 8) {
        const Real c = K.c100;
        const bool bx = fabs_(v.x) > c, by = fabs_(v.y) > c, bz = fabs_(v.z) > c;
        if (__builtin_expect(__any(bx | by | bz), 0)) v = v3(clamp100_(v.x), clamp100_(v.y), clamp100_(v.z));
    } else {
        v = v3(clamp100_(v.x), clamp100_(v.y), clamp100_(v.z));
    }
}

// true where the four prop heights are literal zeros (the compiled-in constants: cf2x_consts); device
// constants, whatever their values, give false
template <typename Real>
__device__ __forceinline__ bool flat_props(const HoverConst<Real>& a) {
    bool flat = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) flat = flat && __builtin_constant_p(a.pz[i]) && a.pz[i] == Real(0);
    return flat;
}

// One Bullet stepSimulation of one drone after the reference's force calls, ω in the body frame
// (st.wb; b.w is not touched: the caller rotates st.wb back once after the last sub-step).  On entry
// st holds the thrust axis, the current z axis, R^T zs and |wb| of the pose b.q; on exit those of the
// new pose.  Returns true if the plane contact model acted.
// K: the chain's literal constants (pinned into VGPRs by the fp64 caller, ChainK)
// EXT: Fext, one more world-frame force through the centre of mass (MultiHoverAviary's downwash), is
// added to the force sum; without it (HoverAviary) the argument is not read
// ROT (plain PYB without EXT): the rotational half alone.  Nothing translational feeds the rotation, so b.pos
// and b.vel are neither read nor written and the plane contact is not tested (returns false).  st.zs and st.zc
// are not formed either (nothing in the rotational half reads them: m3 comes from the increment): whoever runs
// the translational half (pyb_trans_substep) forms them from the quaternions, b.q behind each call
template <typename Real, int PH, bool EXT = false, bool ROT = false>
__device__ __forceinline__ bool pyb_substep(const HoverConst<Real>& a, Body<Real>& b, Chain<Real>& st,
                                            const Real rpm[4], Real sum_f, V3<Real> P, Real tau_z,
                                            const ChainK<Real>& K, V3<Real> Fext = V3<Real>{}, Real* vxy = nullptr) {
    constexpr bool GND = (PH == ADRP_PHYS_PYB_GND || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    constexpr bool DRAG = (PH == ADRP_PHYS_PYB_DRAG || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    constexpr bool FULL = DRAG && !GND;   // the only mode that multiplies by whole matrices
    static_assert(!ROT || (!GND && !DRAG && !EXT), "the rotational half stands alone in plain PYB only");
    // _physics: 4 prop forces + z torque on link 4, LINK_FRAME, cached basis
    const V3<Real> zs = st.zs;
    V3<Real> Fw = v3(sum_f * zs.x, sum_f * zs.y, sum_f * zs.z - a.mass * a.gravity);
    const V3<Real> m3 = st.m3;
    // P x m3 + tau_z m3.  Flat props (literal pz = 0, the compiled-in drone): P.z is +0, and fma(P.y, m3.z,
    // -(0 m3.y)) = P.y m3.z, fma(0, m3.x, c) = c but for the sign of an exact zero, so the two P.z products go
    // (tests/test_hover_offchain_gpu.py holds the compiled kernel to the generic one, which keeps them)
    V3<Real> nb = flat_props(a)
                      ? v3(fmx(tau_z, m3.x, P.y * m3.z), fmx(tau_z, m3.y, -(P.x * m3.z)),
                           fmx(tau_z, m3.z, fmx(P.x, m3.y, -(P.y * m3.x))))
                      : v3(fmx(tau_z, m3.x, fmx(P.y, m3.z, -(P.z * m3.y))), fmx(tau_z, m3.y, fmx(P.z, m3.x, -(P.x * m3.z))),
                           fmx(tau_z, m3.z, fmx(P.x, m3.y, -(P.y * m3.x))));
    if constexpr (GND) {
        // getLinkStates(computeForwardKinematics=1) refreshes the cached basis first (so the drag
        // below is applied in the current basis)
        const Real sqx = b.q.x * b.q.x, sqy = b.q.y * b.q.y, sqz = b.q.z * b.q.z, squ = b.q.w * b.q.w;
        const Real sarg = Real(-2) * (b.q.x * b.q.z - b.q.w * b.q.y);
        const Real den = squ - sqx - sqy + sqz, num = Real(2) * (b.q.y * b.q.z + b.q.w * b.q.x);
        // |roll| < pi/2 and |pitch| < pi/2 of getEulerFromQuaternion (BaseAviary.py:749)
        const bool gate = fabs_(sarg) < Real(0.99999) && (den > Real(0) || (den == Real(0) && num == Real(0)));
        if (gate) {
            Real sg = 0;
            V3<Real> G = v3(Real(0), Real(0), Real(0));
            const V3<Real> r2 = row2_fm(b.q);   // prop heights: the third row of the current pose's matrix
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                Real h = b.pos.z + r2.x * a.px[i] + r2.y * a.py[i] + r2.z * a.pz[i];
                h = h < a.gnd_clip ? a.gnd_clip : h;
                const Real k = a.prop_r4 * rcp_(h);
                const Real g = a.gnd_kf * rpm[i] * rpm[i] * k * k;
                sg += g;
                G = G + v3(g * a.px[i], g * a.py[i], g * a.pz[i]);
            }
            Fw = Fw + sg * st.zc;
            nb = nb + v3(G.y, -G.x, Real(0));
        }
    }
    if constexpr (DRAG) {
        Real s = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) s += b.prev_rpm[i];
        s = s * Real(0.10471975511965977);  // sum(2*pi*rpm/60)
        const V3<Real> dw = v3(-a.drag[0] * s * b.vel.x, -a.drag[1] * s * b.vel.y, -a.drag[2] * s * b.vel.z);
        // np.dot(base_rot.T, drag_factors * vel), applied in the cached link basis
        if constexpr (GND) Fw = Fw + dw;
        else Fw = Fw + mul(st.Rs, mulT(st.R, dw));
    }
    if constexpr (EXT) Fw = Fw + Fext;
    // ---- Bullet: forwardKinematics, ABA of the floating base, semi-implicit Euler ----
    V3<Real> wb = st.wb;
    const V3<Real> Iw = v3(a.ixx * wb.x, a.iyy * wb.y, a.izz * wb.z);
    const Real kw = K.k004 + K.k004 * st.wn;
    // nb - kw Iw - wb x Iw
    const V3<Real> rhs = v3(fmx(wb.z, Iw.y, fmx(-wb.y, Iw.z, fmx(-kw, Iw.x, nb.x))),
                            fmx(wb.x, Iw.z, fmx(-wb.z, Iw.x, fmx(-kw, Iw.y, nb.y))),
                            fmx(wb.y, Iw.x, fmx(-wb.x, Iw.y, fmx(-kw, Iw.z, nb.z))));
    V3<Real> acc{};
    if constexpr (!ROT) {
        const Real kv = K.k004 + K.k004 * hsqrt_nn_(dot(b.vel, b.vel), K);
        acc = v3(fmx(-kv, b.vel.x, a.inv_mass * Fw.x), fmx(-kv, b.vel.y, a.inv_mass * Fw.y),
                 fmx(-kv, b.vel.z, a.inv_mass * Fw.z));
    }
    // ω' = ω + dt R I^-1 rhs in the body frame of the pose the exp map is about to leave: the map
    // rotates about ω' itself, so R'^T ω' = R^T ω' and the body-frame update needs no rotation
    wb = v3(fmx(st.dti.x, rhs.x, wb.x), fmx(st.dti.y, rhs.y, wb.y), fmx(st.dti.z, rhs.z, wb.z));
    if constexpr (!ROT) b.vel = v3(b.vel.x + a.dt * acc.x, b.vel.y + a.dt * acc.y, b.vel.z + a.dt * acc.z);
    Real ang = hsqrt_nn_(dot(wb, wb), K);
    clamp100_body<Real, !ROT>(b.q, wb, ang, b.vel, K);
    st.wb = wb;
    st.wn = ang;
    // (vxy: nothing in a sub-step reads pos.x / pos.y, so the caller may take this sub-step's horizontal
    // velocity instead and run the same two sums itself afterwards, pyb_chain)
    if constexpr (ROT) {
    } else if (vxy) {
        vxy[0] = b.vel.x; vxy[1] = b.vel.y;
        b.pos.z = fmx(a.dt, b.vel.z, b.pos.z);
    } else {
        b.pos = v3(fmx(a.dt, b.vel.x, b.pos.x), fmx(a.dt, b.vel.y, b.pos.y), fmx(a.dt, b.vel.z, b.pos.z));
    }
    // exp-map quaternion update (btMultiBody::stepPositionsMultiDof)
    if (ang > a.ang_max) ang = a.ang_max;          // |w| dt > ANGULAR_MOTION_THRESHOLD
    // sin(|w| dt / 2) / |w| = (dt / 2) sinc(|w| dt / 2): no reciprocal, and Bullet's small-angle
    // form (|w| < 0.001: 0.5 dt - dt^3 |w|^2 / 48) is the same series to rounding
    Real sinc, ch;
    expmap_sinc_cos(Real(0.5) * ang * a.dt, &sinc, &ch, K);
    const Real sc = (Real(0.5) * a.dt) * sinc;
    const V3<Real> ax = sc * wb;
    // (R ax, ch) (x) q0 = q0 (x) (ax, ch): the world-frame increment on the left is the body-frame one on the right
    const Q4<Real> q0 = b.q;
    const Q4<Real> q1 = {ch * q0.x + ax.x * q0.w + ax.z * q0.y - ax.y * q0.z,
                         ch * q0.y + ax.y * q0.w + ax.x * q0.z - ax.z * q0.x,
                         ch * q0.z + ax.z * q0.w + ax.y * q0.x - ax.x * q0.y,
                         ch * q0.w - ax.x * q0.x - ax.y * q0.y - ax.z * q0.z};
    const Real inv = quat_inv_norm(q1.x * q1.x + q1.y * q1.y + q1.z * q1.z + q1.w * q1.w, K);
    // the basis cached by this step's forwardKinematics is the pre-integration pose
    if (a.link_lag) {
        b.ql = q0;
        if constexpr (!ROT) st.zs = st.zc;
        // R'^T col2(R) = third row of the rotation of the increment d = (ax, ch) / |q1|
        const Real s2 = (inv + inv) * inv;
        st.m3 = v3(s2 * (ax.x * ax.z - ch * ax.y), s2 * (ax.y * ax.z + ch * ax.x),
                   Real(1) - s2 * (ax.x * ax.x + ax.y * ax.y));
        if constexpr (FULL) st.Rs = st.R;
    }
    b.q = {q1.x * inv, q1.y * inv, q1.z * inv, q1.w * inv};
    if constexpr (FULL) {
        st.R = rot_fm(b.q);
        st.zc = col2(st.R);
    } else if constexpr (!ROT) {
        st.zc = col2_fm(b.q);
    }
    if (!a.link_lag) {
        if constexpr (!ROT) st.zs = st.zc;
        st.m3 = v3(Real(0), Real(0), Real(1));
        if constexpr (FULL) st.Rs = st.R;
    }
    // plane contact model: non-penetration, no inward velocity.
    // lowest point of the body cylinder: cos(tilt) = R22, sin(tilt) = |(R02, R12)|.  It is at
    // least z + zoff - hh - r below the centre, so a wave whose drones are all higher than that
    // skips the exact test (same result)
    if constexpr (ROT) return false;
    if (__builtin_expect(__any(b.pos.z + a.coll_zoff <= a.coll_hh + a.coll_r + Real(1e-6)), 0)) {
        const Real low = b.pos.z + a.coll_zoff - a.coll_hh * fabs_(st.zc.z) -
                         a.coll_r * hsqrt_nn_(st.zc.x * st.zc.x + st.zc.y * st.zc.y);
        if (low < Real(0)) {
            b.pos.z -= low;
            if (b.vel.z < Real(0)) b.vel.z = Real(0);
            return true;
        }
    }
    return false;
}

// The translational half of pyb_substep<ROT = false> in plain PYB without an external force, for a wave that
// carries pos and vel alone (the hover step's translation wave): the same expressions in the same order, so
// the same bits.  zs: the sub-step's thrust axis.  The plane contact is the caller's (it needs the pose behind
// the sub-step): pyb_trans_contact.
template <typename Real>
__device__ __forceinline__ void pyb_trans_substep(const HoverConst<Real>& a, V3<Real>& pos, V3<Real>& vel, V3<Real> zs,
                                                  Real sum_f, const ChainK<Real>& K) {
    const V3<Real> Fw = v3(sum_f * zs.x, sum_f * zs.y, sum_f * zs.z - a.mass * a.gravity);
    const Real kv = K.k004 + K.k004 * hsqrt_nn_(dot(vel, vel), K);
    const V3<Real> acc = v3(fmx(-kv, vel.x, a.inv_mass * Fw.x), fmx(-kv, vel.y, a.inv_mass * Fw.y),
                            fmx(-kv, vel.z, a.inv_mass * Fw.z));
    vel = v3(vel.x + a.dt * acc.x, vel.y + a.dt * acc.y, vel.z + a.dt * acc.z);
    clamp100_vel(vel, K);
    pos = v3(fmx(a.dt, vel.x, pos.x), fmx(a.dt, vel.y, pos.y), fmx(a.dt, vel.z, pos.z));
}
// pyb_substep's wave-uniform guard of the plane contact test, and the test itself with zc, the third column
// of the pose behind the sub-step
template <typename Real>
__device__ __forceinline__ bool pyb_trans_near_plane(const HoverConst<Real>& a, V3<Real> pos) {
    return __builtin_expect(__any(pos.z + a.coll_zoff <= a.coll_hh + a.coll_r + Real(1e-6)), 0);
}
template <typename Real>
__device__ __forceinline__ bool pyb_trans_contact(const HoverConst<Real>& a, V3<Real>& pos, V3<Real>& vel, V3<Real> zc) {
    const Real low = pos.z + a.coll_zoff - a.coll_hh * fabs_(zc.z) -
                     a.coll_r * hsqrt_nn_(zc.x * zc.x + zc.y * zc.y);
    if (low < Real(0)) {
        pos.z -= low;
        if (vel.z < Real(0)) vel.z = Real(0);
        return true;
    }
    return false;
}

// Physics.DYN (BaseAviary.py:822-896): explicit model, forward Euler, _integrateQ
template <typename Real>
__device__ __forceinline__ void dyn_substep(const HoverConst<Real>& a, Body<Real>& b, const Real rpm[4]) {
    const M3<Real> R = rot(b.q);
    Real f[4], zt[4], sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[i] = rpm[i] * rpm[i] * a.kf;
        zt[i] = rpm[i] * rpm[i] * a.km;
        sum += f[i];
    }
    const V3<Real> zb = col2(R);
    const V3<Real> force_w = v3(sum * zb.x, sum * zb.y, sum * zb.z - a.gravity * a.mass);
    const Real tz = -zt[0] + zt[1] - zt[2] + zt[3];
    const Real tx = (f[0] + f[1] - f[2] - f[3]) * a.dyn_arm;
    const Real ty = (-f[0] + f[1] + f[2] - f[3]) * a.dyn_arm;
    const V3<Real> rr = b.w;
    const V3<Real> tq = v3(tx, ty, tz) - cross(rr, v3(a.ixx * rr.x, a.iyy * rr.y, a.izz * rr.z));
    const V3<Real> rdd = v3(tq.x * a.inv_ixx, tq.y * a.inv_iyy, tq.z * a.inv_izz);
    b.vel = b.vel + a.dt * (a.inv_mass * force_w);
    b.w = rr + a.dt * rdd;
    b.pos = b.pos + a.dt * b.vel;
    const V3<Real> w = b.w;
    const Real wn = hsqrt_(dot(w, w));
    if (!(wn <= Real(1e-8))) {  // np.isclose(omega_norm, 0)
        const Real th = wn * a.dt * Real(0.5);
        Real s, c;
        if (th <= Real(0.39269908169872414)) small_sincos(th, &s, &c);
        else sincos_(th, &s, &c);
        const Real k = s * rcp_(wn);
        const Q4<Real> q = b.q;
        b.q = {c * q.x + k * (w.z * q.y - w.y * q.z + w.x * q.w),
               c * q.y + k * (-w.z * q.x + w.x * q.z + w.y * q.w),
               c * q.z + k * (w.y * q.x - w.x * q.y + w.z * q.w),
               c * q.w + k * (-w.x * q.x - w.y * q.y - w.z * q.z)};
    }
    b.angv = mul(R, b.w);   // resetBaseVelocity(vel, rotation @ rpy_rates)
}

// BaseAviary.reset -> _housekeeping (+ the optional init_noise extension), Real precision
// (a: the reset distribution; gid, tag: the Philox stream of the drone being reset)
template <typename Real>
__device__ __forceinline__ void hover_reset_draw(const HoverReset<Real>& a, uint64_t seed, uint64_t gid, uint32_t tag,
                                                 const HoverConst<Real>& C, Body<Real>& b, int32_t& sc, int32_t& ep) {
    const U4 r0 = draw(seed, gid, uint32_t(ep), tag, 0);
    const U4 r1 = draw(seed, gid, uint32_t(ep), tag, 1);
    const U4 r2 = draw(seed, gid, uint32_t(ep), tag, 2);
    const uint32_t w0[4] = {r0.a, r0.b, r0.c, r0.d}, w1[4] = {r1.a, r1.b, r1.c, r1.d},
                   w2[4] = {r2.a, r2.b, r2.c, r2.d};
    Real p[3], e_[3], v[3], om[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = a.init_xyz[k] + a.n_xyz[k] * (Real(2) * u01r<Real>(w0[k]) - Real(1));
        e_[k] = a.init_rpy[k] + a.n_rpy[k] * (Real(2) * u01r<Real>(w1[k]) - Real(1));
        v[k] = a.n_vel[k] * (Real(2) * u01r<Real>(w2[k]) - Real(1));
    }
    om[0] = a.n_om[0] * (Real(2) * u01r<Real>(w0[3]) - Real(1));
    om[1] = a.n_om[1] * (Real(2) * u01r<Real>(w1[3]) - Real(1));
    om[2] = a.n_om[2] * (Real(2) * u01r<Real>(w2[3]) - Real(1));
    b.q = quat_from_euler_fast<Real>(e_[0], e_[1], e_[2]);
    b.pos = v3(p[0], p[1], p[2]);
    b.ql = b.q;
    b.vel = v3(v[0], v[1], v[2]);
    if (C.physics == ADRP_PHYS_DYN) {
        b.w = mulT(rot(b.q), v3(om[0], om[1], om[2]));
        b.angv = v3(om[0], om[1], om[2]);
    } else {
        b.w = v3(om[0], om[1], om[2]);
        b.angv = v3(Real(0), Real(0), Real(0));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) b.prev_rpm[i] = Real(0);
    sc = 0;
    ep += 1;
}
template <typename Real>
__device__ __forceinline__ void hover_reset_state(const HoverArgs<Real>& args, const HoverConst<Real>& C, int e,
                                                  Body<Real>& b, int32_t& sc, int32_t& ep) {
    hover_reset_draw(*args.r, args.seed, uint64_t(args.env_offset + e), TAG_HOVER_RESET, C, b, sc, ep);
}

// euler_xyz_fast_u's angles one at a time: the same arguments (euler_args, contraction pinned, so the
// same bits) and the same wave-uniform gimbal-lock branch, for the HELP kernel's angle helpers
template <typename Real>
__device__ __forceinline__ Real euler_roll_u(Q4<Real> q) {
    if (__builtin_expect(__any(fabs_(euler_sarg(q)) >= Real(0.99999)), 0)) return euler_xyz_fast(q).x;
    const EulerArgs<Real> a = euler_args(q);
    return fatan2_(a.y0, a.x0);
}
template <typename Real>
__device__ __forceinline__ Real euler_pitch_u(Q4<Real> q) {
    const Real sarg = euler_sarg(q);
    if (__builtin_expect(__any(fabs_(sarg) >= Real(0.99999)), 0)) return euler_xyz_fast(q).y;
    return fasin_(sarg);
}
template <typename Real>
__device__ __forceinline__ Real euler_yaw_u(Q4<Real> q) {
    if (__builtin_expect(__any(fabs_(euler_sarg(q)) >= Real(0.99999)), 0)) return euler_xyz_fast(q).z;
    const EulerArgs<Real> a = euler_args(q);
    return fatan2_(a.y2, a.x2);
}

// The same three for the fp64 angle helper waves, by the lean forms (adrp_device.h, AngK: the wave's pinned
// constants).  One vote sends the whole wave to the function above when any lane is outside the lean forms'
// domain -- NaN, gimbal lock, an atan2 argument pair that is not safely away from zero and infinity -- so
// every input gives the bits it gives above; on the others the lean forms are the same operations.
__device__ __forceinline__ double euler_roll_lean(Q4<double> q, const AngK& k) {
    const EulerArgs<double> a = euler_args(q);
    const bool ok = fabs_(a.sarg) < k.lim && f64::atan2_lean_ok(a.y0, a.x0, k);
    if (__builtin_expect(__any(!ok), 0)) return euler_roll_u(q);
    return f64::atan2_lean<false>(a.y0, a.x0, k);
}
__device__ __forceinline__ double euler_pitch_lean(Q4<double> q, const AngK& k) {
    const double sarg = euler_sarg(q);
    if (__builtin_expect(__any(!(fabs_(sarg) < k.lim)), 0)) return euler_pitch_u(q);
    return f64::asin_lean(sarg, k);
}
__device__ __forceinline__ double euler_yaw_lean(Q4<double> q, const AngK& k) {
    const EulerArgs<double> a = euler_args(q);
    const bool ok = fabs_(a.sarg) < k.lim && f64::atan2_lean_ok(a.y2, a.x2, k);
    if (__builtin_expect(__any(!ok), 0)) return euler_yaw_u(q);
    return f64::atan2_lean<false>(a.y2, a.x2, k);
}

// The chain wave's tilt test without an angle (adrp_device.h, TruncK): false if the lane is unsure, else
// over = |roll| > 0.4 || |pitch| > 0.4 as the float64 angles of euler_xyz_fast_u decide it
__device__ __forceinline__ bool trunc_from_quat(Q4<double> q, const TruncK& k, bool& over) {
    const EulerArgs<double> a = euler_args(q);
    const double as = fabs_(a.sarg), ay = fabs_(a.y0);
    const bool p_over = as > k.s_hi, r_over = ay > k.t_hi * a.x0;
    const bool p_sure = p_over || as < k.s_lo, r_sure = r_over || ay < k.t_lo * a.x0;
    over = p_over || r_over;
    return p_sure && r_sure && a.x0 > 0.0 && as < k.lim;
}
__device__ __forceinline__ bool trunc_from_quat(Q4<float>, const TruncK&, bool&) { return false; }   // (fp64 kernels only)

// E = 1 persistent step (SPLIT): lane L evaluates Euler angle min(L, 2) of the (duplicated) env with
// ONE atan2 -- roll (y0, x0), pitch (sarg, sqrt((1 - sarg)(1 + sarg)), the atan2 form of fasin_),
// yaw (y2, x2) -- and the three come back by readlane: the same arguments as euler_xyz_fast_u
// (euler_args), so the same bits, for one atan2 on the chain instead of three
template <typename Real>
__device__ __forceinline__ Real euler_axis_u(Q4<Real> q, int ax) {
    const EulerArgs<Real> a = euler_args(q);
    const Real sarg = a.sarg;
    if (__builtin_expect(__any(fabs_(sarg) >= Real(0.99999)), 0)) {
        const V3<Real> r = euler_xyz_fast(q);
        return ax == 0 ? r.x : (ax == 1 ? r.y : r.z);
    }
    const Real y0 = a.y0, x0 = a.x0, y2 = a.y2, x2 = a.x2;
    Real x1;
    if constexpr (sizeof(Real) == 8) x1 = f64::sqrt((1.0 - sarg) * (1.0 + sarg));
    else x1 = __builtin_amdgcn_sqrtf((1.0f - sarg) * (1.0f + sarg));
    const Real yy = ax == 0 ? y0 : (ax == 1 ? sarg : y2), xx = ax == 0 ? x0 : (ax == 1 ? x1 : x2);
    return fatan2_(yy, xx);
}
__device__ __forceinline__ float readlane_r(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double readlane_r(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// hover_obs12 with the angles dealt over lanes 0..2 (every lane holds the same env)
template <typename Real>
__device__ __forceinline__ V3<Real> hover_obs12_split(const HoverConst<Real>& a, const Body<Real>& b, float o[12]) {
    const int l = int(threadIdx.x) & 63;
    const Real ang = euler_axis_u(b.q, l < 2 ? l : 2);
    const V3<Real> rpy = v3(readlane_r(ang, 0), readlane_r(ang, 1), readlane_r(ang, 2));
    const V3<Real> w = a.physics == ADRP_PHYS_DYN ? b.angv : b.w;
    o[0] = float(b.pos.x); o[1] = float(b.pos.y); o[2] = float(b.pos.z);
    o[3] = float(rpy.x);   o[4] = float(rpy.y);   o[5] = float(rpy.z);
    o[6] = float(b.vel.x); o[7] = float(b.vel.y); o[8] = float(b.vel.z);
    o[9] = float(w.x);     o[10] = float(w.y);    o[11] = float(w.z);
    return rpy;
}

template <typename Real>
__device__ __forceinline__ V3<Real> hover_obs12(const HoverConst<Real>& a, const Body<Real>& b, float o[12]) {
    const V3<Real> rpy = euler_xyz_fast_u(b.q);
    const V3<Real> w = a.physics == ADRP_PHYS_DYN ? b.angv : b.w;
    o[0] = float(b.pos.x); o[1] = float(b.pos.y); o[2] = float(b.pos.z);
    o[3] = float(rpy.x);   o[4] = float(rpy.y);   o[5] = float(rpy.z);
    o[6] = float(b.vel.x); o[7] = float(b.vel.y); o[8] = float(b.vel.z);
    o[9] = float(w.x);     o[10] = float(w.y);    o[11] = float(w.z);
    return rpy;
}

// one obs row [12 kinematic | B x A action ring, oldest first] from registers
template <int A, int B>
__device__ __forceinline__ void write_row(float* row, const float o12[12], const float (&ring)[B][A], int head1) {
    if constexpr (A == 4) {
        float4* r4 = reinterpret_cast<float4*>(row);
        r4[0] = make_float4(o12[0], o12[1], o12[2], o12[3]);
        r4[1] = make_float4(o12[4], o12[5], o12[6], o12[7]);
        r4[2] = make_float4(o12[8], o12[9], o12[10], o12[11]);
#pragma unroll
        for (int p = 0; p < B; ++p) {          // physical slot p -> logical position k
            int k = p - head1;
            k += k < 0 ? B : 0;
            r4[3 + k] = make_float4(ring[p][0], ring[p][1], ring[p][2], ring[p][3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) row[k] = o12[k];
#pragma unroll
        for (int p = 0; p < B; ++p) {
            int k = p - head1;
            k += k < 0 ? B : 0;
#pragma unroll
            for (int j = 0; j < A; ++j) row[12 + k * A + j] = ring[p][j];
        }
    }
}

// generic-B variant: the ring part is copied from HBM in logical order (slot head1 = oldest);
// the newest entry (logical B-1) is this step's action
template <int A>
__device__ __forceinline__ void write_row_generic(float* __restrict__ row, const float o12[12],
                                                  const float* __restrict__ ring, int B, int E, int e, int head1,
                                                  const float act[A], bool act_is_newest) {
#pragma unroll
    for (int k = 0; k < 12; ++k) row[k] = o12[k];
    // chunks of 8 slots: all loads of a chunk in flight before its stores
    constexpr int CH = 8;
    int slot = head1;
    for (int k0 = 0; k0 < B; k0 += CH) {
        float v[CH][A];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int k = k0 + c;
#pragma unroll
            for (int j = 0; j < A; ++j)
                v[c][j] = k < B ? ((act_is_newest && k == B - 1) ? act[j] : ring[(size_t(slot) * E + e) * A + j]) : 0.0f;
            slot = slot + 1 == B ? 0 : slot + 1;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int k = k0 + c;
            if (k < B)
#pragma unroll
                for (int j = 0; j < A; ++j) row[12 + k * A + j] = v[c][j];
        }
    }
}

// DSLPIDControl.computeControl (control/DSLPIDControl.py:82-259) for the HoverAviary PID / VEL /
// ONE_D_PID action types (BaseRLAviary.py:193-235): once per env.step, on the state at the
// start of the step.  ctl = last_rpy 3, integral_pos_e 3, integral_rpy_e 3 (in/out).  The
// scipy Euler round trip of the target rotation (:205, :242-244) is the identity on a proper
// rotation, so the target basis is used directly (oracle/oracle.c orc_dslpid, pinned by
// tests/golden/pid_golden.npz).
template <typename Real, int CTL>
__device__ __forceinline__ void dslpid_rpm(const HoverConst<Real>& C, const Body<Real>& b, const float* act,
                                           Real ctl[HF_NPID], Real rpm[4]) {
    const M3<Real> R = rot(b.q);
    const V3<Real> rpy = euler_xyz(b.q);   // accurate: the D term scales its error by 6e5
    V3<Real> tp, tv = v3(Real(0), Real(0), Real(0));
    Real tyaw = 0;
    if constexpr (CTL == ADRP_ACT_PID) {
        // _calculateNextStep(pos, action, step_size=1) (BaseAviary.py:1112-1160)
        const V3<Real> d = v3(Real(act[0]) - b.pos.x, Real(act[1]) - b.pos.y, Real(act[2]) - b.pos.z);
        const Real dist = sqrt_(dot(d, d));
        tp = dist <= Real(1) ? v3(Real(act[0]), Real(act[1]), Real(act[2])) : b.pos + (Real(1) / dist) * d;
    } else if constexpr (CTL == ADRP_ACT_VEL) {
        // target_vel = SPEED_LIMIT*|a3|*a[0:3]/|a[0:3]| in float32 (float32 action, NEP 50)
#pragma clang fp contract(off)
        tp = b.pos;
        tyaw = rpy.z;
        // correctly rounded float32 sqrt / division through float64 (53 >= 2*24 + 2 bits)
        const float n = float(sqrt(double(act[0] * act[0] + act[1] * act[1] + act[2] * act[2])));
        const float s = C.speed_limit * fabsf(act[3]);
        if (n != 0.0f) {
            const double dn = double(n);
            tv = v3(Real(s * float(double(act[0]) / dn)), Real(s * float(double(act[1]) / dn)),
                    Real(s * float(double(act[2]) / dn)));
        }
    } else {   // ONE_D_PID: target_pos = pos + 0.1*[0, 0, a]
        tp = v3(b.pos.x, b.pos.y, b.pos.z + Real(0.1) * Real(act[0]));
    }
    // the two loops (dslpid_core.h) with DSLPIDControl's CF2X gains (:42-47) and no target rates
    constexpr DslpidGains<Real> K = {{Real(.4), Real(.4), Real(1.25)}, {Real(.05), Real(.05), Real(.05)},
                                     {Real(.2), Real(.2), Real(.5)}, {Real(70000), Real(70000), Real(60000)},
                                     {Real(0), Real(0), Real(500)}, {Real(20000), Real(20000), Real(12000)}};
    const Real tpa[3] = {tp.x, tp.y, tp.z}, tva[3] = {tv.x, tv.y, tv.z}, rates[3] = {Real(0), Real(0), Real(0)};
    Real thrust, tq[3], pos_e[3], tt[3];
    V3<Real> xax, yax;
    dslpid_core<Real>(K, C.ctrl_dt, C.ctrl_hz, C.pid_grav, C.pid_inv4kf, Real(4070.3), Real(1.0 / 0.2685), R, rpy, b.pos,
                      b.vel, tpa, tyaw, tva, rates, ctl, thrust, tq, pos_e, tt, xax, yax);
    // CF2X mixer [[-.5,-.5,-1],[-.5,.5,1],[.5,.5,-1],[.5,-.5,1]], PWM clip, PWM -> RPM
    const Real hr = Real(0.5) * tq[0], hp = Real(0.5) * tq[1];
    const Real pwm[4] = {thrust - hr - hp - tq[2], thrust - hr + hp + tq[2], thrust + hr + hp - tq[2],
                         thrust + hr - hp + tq[2]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Real p = pwm[i] < Real(20000) ? Real(20000) : (pwm[i] > Real(65535) ? Real(65535) : pwm[i]);
        rpm[i] = Real(0.2685) * p + Real(4070.3);
    }
}

// ---- state field addressing ----
// The state is [field][E]: field k of env e lies k * E * sizeof(T) bytes behind the env's field 0.  Indexed
// as f[k * E + e] every field costs three VALU instructions (add, sign extension, 64-bit shift-add) and
// a 64-bit address pair that lives from the loads to the stores.  Here a lane walks the fields with ONE
// 32-bit byte offset on the uniform base pointer, the saddr + voffset form of the global instructions: a
// v_add_u32 of the stride per field, and the offsets (one VGPR each) serve the stores again.  (field_lane:
// the offset is opaque to the optimiser, which would otherwise rebuild off0 + k * stride per field.)
// The offsets are 32-bit, so the form holds while every field of the block, the PID fields included, ends
// below 4 GiB: up to kFieldOffsetMaxBytes / ((HF_NBASE + HF_NPID) sizeof(T)) envs (field_offsets_fit;
// adrp_internal.h states the bound).  Above it the accesses keep 64-bit indices: the hover step kernel
// has both forms and the host picks one (W32); the other callers of load_body / store_body branch on E.
constexpr uint64_t kFieldOffsetMaxBytes = uint64_t(1) << 32;
template <typename T>
__host__ __device__ constexpr uint32_t field_offsets_max_envs() {
    return uint32_t(kFieldOffsetMaxBytes / (uint64_t(HF_NBASE + HF_NPID) * sizeof(T)));
}
template <typename T>
__host__ __device__ constexpr bool field_offsets_fit(int E) {
    return __builtin_expect(uint32_t(E) <= field_offsets_max_envs<T>(), 1);
}
__device__ __forceinline__ uint32_t field_lane(uint32_t off) {
    asm("" : "+v"(off));
    return off;
}
// keeps the value's uses behind (and its definition before) the side-effecting statements around it
__device__ __forceinline__ void hold(double& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void hold(float& x) { asm volatile("" : "+v"(x)); }
// Ends the 32-bit arm of a branch on field_offsets_fit.  Both arms finish with the same loads (or stores)
// of the same fields; without a difference at their ends the optimiser sinks those into the join with the
// address picked per field from the two forms (a 64-bit select each), which is worse than either.
__device__ __forceinline__ void field_form_end() { asm volatile(""); }
template <typename T>
__device__ __forceinline__ T& field_at(T* base, uint32_t off) {
    return *(T*)((const char*)base + off);   // (T may be const: the byte pointer drops it for the arithmetic only)
}
// the last use of an offset (the stores): the address is formed behind a statement that stays in the
// store's own block, so it is not shared with the load's block as a 64-bit pair formed above both
template <typename T>
__device__ __forceinline__ T& field_last(T* base, uint32_t off) {
    asm volatile("" : "+v"(off));
    return *(T*)((const char*)base + off);
}
// byte offsets o[first .. first + n) of the lane's fields first .. first + n - 1 (off0: of its field 0)
template <int N>
__device__ __forceinline__ void field_run(uint32_t off0, uint32_t stride, int first, int n, uint32_t (&o)[N]) {
    uint32_t off = first ? field_lane(off0 + uint32_t(first) * stride) : off0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        o[first + i] = off;
        if (i + 1 < n) off = field_lane(off + stride);
    }
}
// the offsets of one env's Body fields (those the mode reads; the others stay unset and unused)
template <typename Real>
struct BodyOffs {
    uint32_t o[HF_NBASE];
};
template <typename Real>
__device__ __forceinline__ BodyOffs<Real> body_offsets(int E, int e, bool lag, bool drag, bool dyn) {
    BodyOffs<Real> r;
    const uint32_t stride = uint32_t(E) * uint32_t(sizeof(Real)), off0 = uint32_t(e) * uint32_t(sizeof(Real));
    field_run(off0, stride, HF_POS, HF_LAST_RPM - HF_POS, r.o);   // pos, quat, vel, omega
    if (drag) field_run(off0, stride, HF_LAST_RPM, 4, r.o);
    if (dyn) field_run(off0, stride, HF_ANGV, 3, r.o);
    if (lag) field_run(off0, stride, HF_LINK_QUAT, 4, r.o);
    return r;
}

// (kin = false: pos and vel are another wave's to load; they are left zero)
template <typename Real>
__device__ __forceinline__ void load_body_at(const Real* f, const BodyOffs<Real>& k, Body<Real>& b, bool lag,
                                             bool drag, bool dyn, bool kin = true) {
    if (kin) b.pos = v3(field_at(f, k.o[HF_POS + 0]), field_at(f, k.o[HF_POS + 1]), field_at(f, k.o[HF_POS + 2]));
    else b.pos = v3(Real(0), Real(0), Real(0));
    b.q = {field_at(f, k.o[HF_QUAT + 0]), field_at(f, k.o[HF_QUAT + 1]), field_at(f, k.o[HF_QUAT + 2]),
           field_at(f, k.o[HF_QUAT + 3])};
    if (kin) b.vel = v3(field_at(f, k.o[HF_VEL + 0]), field_at(f, k.o[HF_VEL + 1]), field_at(f, k.o[HF_VEL + 2]));
    else b.vel = v3(Real(0), Real(0), Real(0));
    b.w = v3(field_at(f, k.o[HF_OMEGA + 0]), field_at(f, k.o[HF_OMEGA + 1]), field_at(f, k.o[HF_OMEGA + 2]));
    if (lag) b.ql = {field_at(f, k.o[HF_LINK_QUAT + 0]), field_at(f, k.o[HF_LINK_QUAT + 1]),
                     field_at(f, k.o[HF_LINK_QUAT + 2]), field_at(f, k.o[HF_LINK_QUAT + 3])};
    else b.ql = b.q;
#pragma unroll
    for (int i = 0; i < 4; ++i) b.prev_rpm[i] = drag ? field_at(f, k.o[HF_LAST_RPM + i]) : Real(0);
    if (dyn) b.angv = v3(field_at(f, k.o[HF_ANGV + 0]), field_at(f, k.o[HF_ANGV + 1]), field_at(f, k.o[HF_ANGV + 2]));
    else b.angv = v3(Real(0), Real(0), Real(0));
}
template <typename Real>
__device__ __forceinline__ void store_body_at(Real* f, const BodyOffs<Real>& k, const Body<Real>& b, bool lag,
                                              bool drag, bool dyn) {
    field_last(f, k.o[HF_POS + 0]) = b.pos.x; field_last(f, k.o[HF_POS + 1]) = b.pos.y; field_last(f, k.o[HF_POS + 2]) = b.pos.z;
    field_last(f, k.o[HF_QUAT + 0]) = b.q.x; field_last(f, k.o[HF_QUAT + 1]) = b.q.y;
    field_last(f, k.o[HF_QUAT + 2]) = b.q.z; field_last(f, k.o[HF_QUAT + 3]) = b.q.w;
    field_last(f, k.o[HF_VEL + 0]) = b.vel.x; field_last(f, k.o[HF_VEL + 1]) = b.vel.y; field_last(f, k.o[HF_VEL + 2]) = b.vel.z;
    field_last(f, k.o[HF_OMEGA + 0]) = b.w.x; field_last(f, k.o[HF_OMEGA + 1]) = b.w.y; field_last(f, k.o[HF_OMEGA + 2]) = b.w.z;
    if (lag) {
        field_last(f, k.o[HF_LINK_QUAT + 0]) = b.ql.x; field_last(f, k.o[HF_LINK_QUAT + 1]) = b.ql.y;
        field_last(f, k.o[HF_LINK_QUAT + 2]) = b.ql.z; field_last(f, k.o[HF_LINK_QUAT + 3]) = b.ql.w;
    }
    if (drag) {
#pragma unroll
        for (int i = 0; i < 4; ++i) field_last(f, k.o[HF_LAST_RPM + i]) = b.prev_rpm[i];
    }
    if (dyn) {
        field_last(f, k.o[HF_ANGV + 0]) = b.angv.x; field_last(f, k.o[HF_ANGV + 1]) = b.angv.y;
        field_last(f, k.o[HF_ANGV + 2]) = b.angv.z;
    }
}

template <typename Real>
__device__ __forceinline__ void load_body(const HoverArgs<Real>& a, int e, Body<Real>& b, bool lag, bool drag,
                                          bool dyn) {
    const int E = a.E;
    const Real* f = a.f;
    if (field_offsets_fit<Real>(E)) {
        load_body_at(f, body_offsets<Real>(E, e, lag, drag, dyn), b, lag, drag, dyn);
        field_form_end();
        return;
    }
    b.pos = v3(f[(HF_POS + 0) * E + e], f[(HF_POS + 1) * E + e], f[(HF_POS + 2) * E + e]);
    b.q = {f[(HF_QUAT + 0) * E + e], f[(HF_QUAT + 1) * E + e], f[(HF_QUAT + 2) * E + e], f[(HF_QUAT + 3) * E + e]};
    b.vel = v3(f[(HF_VEL + 0) * E + e], f[(HF_VEL + 1) * E + e], f[(HF_VEL + 2) * E + e]);
    b.w = v3(f[(HF_OMEGA + 0) * E + e], f[(HF_OMEGA + 1) * E + e], f[(HF_OMEGA + 2) * E + e]);
    if (lag) b.ql = {f[(HF_LINK_QUAT + 0) * E + e], f[(HF_LINK_QUAT + 1) * E + e], f[(HF_LINK_QUAT + 2) * E + e],
                     f[(HF_LINK_QUAT + 3) * E + e]};
    else b.ql = b.q;
#pragma unroll
    for (int i = 0; i < 4; ++i) b.prev_rpm[i] = drag ? f[(HF_LAST_RPM + i) * E + e] : Real(0);
    if (dyn) b.angv = v3(f[(HF_ANGV + 0) * E + e], f[(HF_ANGV + 1) * E + e], f[(HF_ANGV + 2) * E + e]);
    else b.angv = v3(Real(0), Real(0), Real(0));
}

template <typename Real>
__device__ __forceinline__ void store_body(const HoverArgs<Real>& a, int e, const Body<Real>& b, bool lag,
                                           bool drag, bool dyn) {
    const int E = a.E;
    Real* f = a.f;
    if (field_offsets_fit<Real>(E)) {
        store_body_at(f, body_offsets<Real>(E, e, lag, drag, dyn), b, lag, drag, dyn);
        field_form_end();
        return;
    }
    f[(HF_POS + 0) * E + e] = b.pos.x; f[(HF_POS + 1) * E + e] = b.pos.y; f[(HF_POS + 2) * E + e] = b.pos.z;
    f[(HF_QUAT + 0) * E + e] = b.q.x; f[(HF_QUAT + 1) * E + e] = b.q.y;
    f[(HF_QUAT + 2) * E + e] = b.q.z; f[(HF_QUAT + 3) * E + e] = b.q.w;
    f[(HF_VEL + 0) * E + e] = b.vel.x; f[(HF_VEL + 1) * E + e] = b.vel.y; f[(HF_VEL + 2) * E + e] = b.vel.z;
    f[(HF_OMEGA + 0) * E + e] = b.w.x; f[(HF_OMEGA + 1) * E + e] = b.w.y; f[(HF_OMEGA + 2) * E + e] = b.w.z;
    if (lag) {
        f[(HF_LINK_QUAT + 0) * E + e] = b.ql.x; f[(HF_LINK_QUAT + 1) * E + e] = b.ql.y;
        f[(HF_LINK_QUAT + 2) * E + e] = b.ql.z; f[(HF_LINK_QUAT + 3) * E + e] = b.ql.w;
    }
    if (drag) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[(HF_LAST_RPM + i) * E + e] = b.prev_rpm[i];
    }
    if (dyn) {
        f[(HF_ANGV + 0) * E + e] = b.angv.x; f[(HF_ANGV + 1) * E + e] = b.angv.y; f[(HF_ANGV + 2) * E + e] = b.angv.z;
    }
}

// The PYB sub-step chain of one env.step of one drone: the prop force sums of the step's RPMs, ω and the
// thrust axis into the body frame, S sub-steps (SC > 0: compile-time count, unrolled), ω back to the
// world frame.  ext(b, st), unless NoExtForce, gives each sub-step one more world-frame force from the
// state at its start (every lane of the wave calls it: it may exchange across lanes).  Returns true if
// the plane contact model acted.
// hand, unless NoHandOff (plain PYB, no external force, SC > 0): the chain runs the rotational half of every
// sub-step alone (pyb_substep<ROT>; b.pos and b.vel are not touched, false is returned) and hands the quaternions
// of its poses to whoever runs the translational half, who forms their third columns, col2_fm(q): pose k = s + 2
// is b.q behind sub-step s, hand.pose(s + 2, b.q).  Sub-step s takes its thrust axis from pose s with the link
// lag, from pose s + 1 without, and its contact test from pose s + 2; poses 0 and 1 are b.ql and b.q as loaded,
// which the receiver loads itself.  The pre-loop still forms zs once, for m3.  hand.head(), once ahead of the
// sub-steps, stores nothing: it is the chain's side of the receiver's start (a barrier).  The chain only hands
// out: it never waits for the other side.
struct NoExtForce {};
struct NoHandOff {};
// What a step's four RPMs give every sub-step: the prop force sum (the thrust along the thrust axis), the
// forces' moment arm sum P and the z torque.  (A caller that needs the force sum alone, the hover step's
// translation wave, reads that member alone: the same statements, so the same bits.)
template <typename Real>
struct PropSums {
    Real sum_f, tau_z;
    V3<Real> P;
};
template <typename Real>
__device__ __forceinline__ PropSums<Real> prop_sums(const HoverConst<Real>& C, const Real rpm[4]) {
    Real sum_f = 0, t2 = 0;
    V3<Real> P = v3(Real(0), Real(0), Real(0));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Real r2 = rpm[i] * rpm[i];
        const Real f = r2 * C.kf;
        sum_f += f;
        // the reference drone's props sit in the body plane: a literal pz = 0 adds f * 0 = +0 (f >= 0) to
        // +0, so P.z stays +0 without the multiply-adds (race_pyb_substep_r's idiom; flat_props below)
        const bool pz0 = __builtin_constant_p(C.pz[i]) && C.pz[i] == Real(0);
        const Real fx = f * C.px[i], fy = f * C.py[i], fz = f * C.pz[i];   // (products and sums in separate
        P = v3(P.x + fx, P.y + fy, pz0 ? P.z : P.z + fz);                  //  statements: no contraction, as before)
        t2 += (i & 1) ? -r2 : r2;
    }
    return {sum_f, t2 * C.km, P};    // tau_z = KM*(rpm0^2 - rpm1^2 + rpm2^2 - rpm3^2), IROS sign
}
template <typename Real, int PH, int SC, bool DRAG, typename Ext, typename Hand = NoHandOff>
__device__ __forceinline__ bool pyb_chain(const HoverConst<Real>& C, Body<Real>& b, const Real rpm_in[4], bool lag,
                                          Ext ext, V3<Real>* wb_out = nullptr, Real* vxy = nullptr, Hand hand = Hand{}) {
    constexpr bool EXT = !__is_same(Ext, NoExtForce);
    constexpr bool HAND = !__is_same(Hand, NoHandOff);
    static_assert(!HAND || (!EXT && !DRAG && SC > 0 && PH == ADRP_PHYS_PYB), "the hand-off is plain PYB's");
    // (a local copy: nothing the sub-steps store can alias it, so what depends on the RPMs alone is
    // computed once for the unrolled sub-steps)
    const Real rpm[4] = {rpm_in[0], rpm_in[1], rpm_in[2], rpm_in[3]};
    const PropSums<Real> ps = prop_sums(C, rpm);
    const Real sum_f = ps.sum_f, tau_z = ps.tau_z;
    const V3<Real> P = ps.P;
    // the chain's constants in VGPRs for the whole loop (fp64: no 64-bit literal operands)
    ChainK<Real> K = chain_consts<Real>();
    HoverConst<Real> Cp = C;
    if constexpr (sizeof(Real) == 8) {
        pin_all(K);
        // (HAND: mass, gravity, inv_mass and coll_* are the translational half's alone; leaving their pins out
        // here measured no gain by the A/B rule, profiles/ab_hover_transwave.txt, so the list stays one)
        pin(Cp.dt); pin(Cp.mass); pin(Cp.gravity); pin(Cp.inv_mass); pin(Cp.ang_max);
        pin(Cp.ixx); pin(Cp.iyy); pin(Cp.izz); pin(Cp.inv_ixx); pin(Cp.inv_iyy); pin(Cp.inv_izz);
        pin(Cp.coll_hh); pin(Cp.coll_r); pin(Cp.coll_zoff);
    }
    // into the body frame: ω, the thrust axis (third column of the cached link basis) and its
    // body coordinates; the loop carries these, not the matrices
    Chain<Real> st{};
    {
        const M3<Real> R = rot_fm(b.q);
        const M3<Real> Rs = lag ? rot_fm(b.ql) : R;
        st.wb = mulT(R, b.w);
        st.zc = col2(R);
        st.zs = col2(Rs);
        st.m3 = lag ? mulT(R, st.zs) : v3(Real(0), Real(0), Real(1));
        if constexpr (DRAG) {
            st.R = R;
            st.Rs = Rs;
        }
    }
    st.wn = hsqrt_nn_(dot(b.w, b.w), K);
    st.dti = v3(Cp.dt * Cp.inv_ixx, Cp.dt * Cp.inv_iyy, Cp.dt * Cp.inv_izz);
    if constexpr (HAND) hand.head();
    bool touched = false;
    // vxy (SC > 0, no external force): the horizontal position is left at its value before the chain and the
    // SC sub-steps' horizontal velocities come back in vxy[2 s], vxy[2 s + 1]: the caller runs
    // pos.x = fma(dt, vxy[2 s], pos.x), likewise y, in order (pos_xy_sums: the same operations, the same bits)
    auto substep = [&](int s) {
        if constexpr (HAND) {
            pyb_substep<Real, PH, false, true>(Cp, b, st, rpm, sum_f, P, tau_z, K);
            hand.pose(s + 2, b.q);
        } else if constexpr (EXT) touched |= pyb_substep<Real, PH, true>(Cp, b, st, rpm, sum_f, P, tau_z, K, ext(b, st));
        else touched |= pyb_substep<Real, PH>(Cp, b, st, rpm, sum_f, P, tau_z, K, V3<Real>{}, vxy ? vxy + 2 * s : nullptr);
#pragma unroll
        for (int i = 0; i < 4; ++i) b.prev_rpm[i] = rpm[i];  // last_clipped_action
    };
    if constexpr (SC > 0) {
#pragma unroll
        for (int s = 0; s < SC; ++s) substep(s);
    } else {
        for (int s = 0; s < C.S; ++s) substep(s);
    }
    // state, obs and the stored link_quat stay in the world frame (wb_out: the caller rotates back itself,
    // b.w = rot_fm(b.q) wb, where it has a wait to fill)
    if (wb_out) *wb_out = st.wb;
    else b.w = mul(rot_fm(b.q), st.wb);
    return touched;
}

}  // namespace adrp
