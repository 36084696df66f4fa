// hover_kernel.h — fused HoverAviary env.step for gfx950: one lane per env, all
// PYB_FREQ/CTRL_FREQ sub-steps in registers, then obs / reward / terminated /
// truncated and (optionally) the VecEnv auto-reset, in ONE launch.
//
// Reference path (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08):
//   BaseAviary.step            envs/BaseAviary.py:262-387 (sub-step loop 347-376)
//   _preprocessAction          envs/BaseRLAviary.py:160-239 (RPM 192, ONE_D_RPM 225)
//   _physics / _groundEffect / _drag / _downwash   envs/BaseAviary.py:683-818
//   p.stepSimulation (Bullet btMultiBody floating base)        BaseAviary.py:373-374
//   _dynamics / _integrateQ (Physics.DYN)          envs/BaseAviary.py:822-896
//   _computeObs                envs/BaseRLAviary.py:284-319
//   _computeReward / _computeTerminated / _computeTruncated    envs/HoverAviary.py:68-117
//
// The dynamics (the closed form of a Bullet sub-step, the sub-step chain, the reset draw, the obs row and
// the state's field addressing) are hover_dynamics.h's, shared with the multi-hover, ctrl and persistent
// kernels.  This file is the step kernel: one function per wave role and the dispatcher over them.
//
// Latency design (E = 4096 is 64 waves on 256 CUs: the kernel is one wave's critical
// path): no divides or IEEE sqrt in the sub-step chain (reciprocal constants, 1-ulp
// hardware rcp/sqrt/rsq), small-angle sin/cos polynomial, the lagged thrust axis is the
// previous sub-step's z axis (carried, not recomputed), the state fields are addressed by one
// 32-bit offset each on the scalar base (body_offsets) and loaded first, the action-ring loads
// are issued at entry independent of the ring head, rows are written with 16-byte
// per-lane stores straight from registers (no LDS, no barrier) or, staged kernels, leave as one
// coalesced block with the helper waves (HELP) taking the ring, the resets and the obs angles.
#pragma once

#include "hover_dynamics.h"

namespace adrp {

// ------------------------------------------------------------------------------------------
// env.step kernel: lane = env; B (ring length) is a template parameter so the ring lives
// in registers
// ------------------------------------------------------------------------------------------
constexpr int kResetFields = 16; // pos 3, quat 4, vel 3, w 3, angv 3 of a reset state (HELP)
// obs rows staged in LDS, then written as one contiguous, fully coalesced block of
// 64 rows (the row-per-lane float4 stores leave partial 64-B lines: +18 % write traffic)
constexpr int kRowF4 = 18;        // 72 floats = 18 float4 per obs row (A = 4, B = 15)
constexpr int kResetObs = kStepBlock * kRowF4;   // ANG: behind the 64 rows, the reset obs as three float4 per env
// fp64 HELP kernels: two more helper waves beside the reset helper compute the obs row's pitch and yaw
// from the chain's final quaternion, and the reset helper, idle by then, the roll; the chain meanwhile
// rotates ω back to the world frame, converts the row and computes the reward
// (float64 only: in float32 the two extra barriers cost more than the two atan2 they take off the
// chain, +1.2 % against -1.2 % in float64, A/B round 6)
template <typename Real>
constexpr bool angle_helpers() { return sizeof(Real) == 8; }
template <typename Real>
constexpr int help_waves() { return angle_helpers<Real>() ? 3 : 1; }   // helper waves of a HELP workgroup

// The quaternion slots of the pose hand-off and their marks (a view of StepLds's tw_q / tw_mark), TW kernels.
// With plain PYB and no external force the translational half of a sub-step (force, |v|, velocity and its
// clamp, position, plane contact) feeds nothing back into the rotation; all it takes from there is the thrust
// axis, which with the link lag is the z axis of the pose TWO sub-steps back.  Wave 3, the yaw helper,
// otherwise idle before barrier A, runs that half for the chain's lanes (hover_trans_wave):
//   the chain (pyb_chain's hand-off) writes the quaternion of each of its poses, which it holds anyway for the
//   next quaternion product, into slot k as two 16-byte halves (k = s + 2: the pose behind sub-step s), then
//   mark[k].  It only writes: no load of pos / vel, no wait, no poll before A.  One wave's LDS operations
//   complete in order, so the mark is visible after the data.  (LDS keeps whatever the last workgroup on the
//   CU left: wave 3 clears the marks and waits for the clears to land ahead of a bare s_barrier that the helper
//   waves pass at their head and the chain wave ahead of its first slot write: the head barrier.)
//   wave 3 forms the z axis at each read, thrust axis and contact test alike: col2_fm, the chain's own
//   expression on the chain's own bits.  Slots 0 and 1, the cached link basis and the pose at entry, are state
//   fields as loaded: wave 3 loads them itself beside pos / vel and needs no mark for them, q holds slots
//   2 .. SC + 1 alone.
// The marks are one word per slot, never per lane or per value: a NaN, gimbal-lock or clamped lane is stored
// and marked like any other.  Nobody waits forever: wave 3's clear of all kSlots mark words lands before the
// head barrier and no mark is written ahead of that barrier; behind it the chain writes every one of its marks
// without a wait, a poll or a barrier of its own before A, and wave 3 waits for chain marks alone.  The wait
// graph is chain -> wave 3, no cycle, and every polling wave reaches A whatever the data holds.
// The marks are relaxed workgroup-scope atomics (plain ds_read / ds_write, no s_waitcnt of their own); the
// empty asm keeps the compiler from moving the data accesses across them, the LDS keeps a wave's order.
template <typename Real, int SC>
struct PoseSlots {
    using Real2 = Real __attribute__((ext_vector_type(2)));
    static constexpr int kSlots = SC + 2;
    Real2* q;     // [2 (k - 2) + half][lane]
    int* mark;    // [k]
    // wave 3, ahead of the head barrier: the marks cleared, and the clears landed
    __device__ __forceinline__ void clear(int tl) const {
        if (tl < kSlots) __hip_atomic_store(&mark[tl], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the clears are in LDS
    }
    // The head barrier: no mark of this launch is written before every clear.  The chain's sits ahead of its
    // first LDS write and behind its loads and the pre-loop: the translation wave's lgkmcnt(0) in front of the
    // barrier also covers that wave's kernel-argument loads, which come in cold (later than the chain's state
    // loads), and by now they have
    __device__ __forceinline__ static void head() { __builtin_amdgcn_s_barrier(); }
    __device__ __forceinline__ void wait(int k) const {   // one LDS word per poll; the chain wave is co-resident and always arrives
        while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&mark[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0)
            __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ V3<Real> zaxis(int k, int tl) const {   // the z axis of the pose in slot k
        const Real2 xy = q[(2 * k - 4) * kStepBlock + tl], zw = q[(2 * k - 3) * kStepBlock + tl];
        return col2_fm(Q4<Real>{Real(xy.x), Real(xy.y), Real(zw.x), Real(zw.y)});
    }
    __device__ __forceinline__ void pose(int k, Q4<Real> p) const {   // the chain wave's hand-off (stores only)
        const int tl = threadIdx.x;
        Real2 xy, zw;
        xy.x = p.x; xy.y = p.y; zw.x = p.z; zw.y = p.w;
        q[(2 * k - 4) * kStepBlock + tl] = xy;
        q[(2 * k - 3) * kStepBlock + tl] = zw;
        asm volatile("" ::: "memory");
        __hip_atomic_store(&mark[k], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// The step kernel's LDS, by what sizes it.
//   rows       STG: the 64 staged obs rows; ANG: behind them the reset obs of the block's envs as three float4
//              per env (kResetObs), which the helper waves' copy-out takes whole
//   rs_body    HELP: the reset helper's next-episode states, [kResetFields][lane]; rs_obs: their obs (fp32)
//   ang_*      ANG: the chain's final quaternion for the angle helpers, and their angles back for the unsure
//              tilt test.  TW kernels keep the quaternion in the four rows of tw_out that were unused, so that
//              three workgroups still fit the CU's 160 KB
//   done_*     ANG: one byte per lane (the env is done), the done lanes at their rank, their count
//   tw_*       TW: PoseSlots' storage; the translation wave's final pos / vel, indexed as rs_body is (the chain
//              takes the six values behind A from there or, for a done lane, from rs_body), and its flag byte
//              per lane: terminated, a position limit passed
// A view: the arrays themselves are hover_step_body's __shared__ variables, one each, so that a kernel's LDS is
// what it uses and every array keeps an address of its own for the instructions' offset fields (as one object
// of this struct the 22 ANG kernels without a translation wave took 8 bytes more, the size rounded up to the
// rows' alignment, and the chain's tail formed its lane offsets again per array).
template <typename Real, int SC, bool STG, bool HELP, bool ANG, bool TW>
struct StepLds {
    using Slots = PoseSlots<Real, SC>;
    static constexpr int kTwOut = HF_VEL + 3;
    static constexpr int kRows = STG ? kStepBlock * kRowF4 + (ANG ? 3 * kStepBlock : 0) : 1;
    float4* rows;
    typename Slots::Real2* tw_q;
    Real *rs_body, *tw_out, *ang_q_own, *ang_r, *ang_p;
    float *rs_obs, *ang_y;
    int *done_cnt, *tw_mark;
    uint8_t *done_list, *done_b, *tw_flag;
#ifdef ADRP_RACE_TIMING
    unsigned long long* tw_time;
#endif

    __device__ __forceinline__ Slots slots() { return {tw_q, tw_mark}; }
    __device__ __forceinline__ Real* ang_q() {
        if constexpr (TW) return tw_out + HF_QUAT * kStepBlock;
        else return ang_q_own;
    }
    __device__ __forceinline__ Q4<Real> ang_q_read(int tl) {
        Real* const p = ang_q();
        return {p[tl], p[kStepBlock + tl], p[2 * kStepBlock + tl], p[3 * kStepBlock + tl]};
    }
    __device__ __forceinline__ void ang_q_write(int tl, Q4<Real> v) {
        Real* const p = ang_q();
        p[tl] = v.x; p[kStepBlock + tl] = v.y; p[2 * kStepBlock + tl] = v.z;
        p[3 * kStepBlock + tl] = v.w;
    }
};

// B == 0: runtime ring length a.B;  SC > 0: compile-time sub-step count (loop fully unrolled);
// STG: LDS-staged obs rows (needs A == 4, B == 15 and every lane of the block live);
// CTL: 0 (RPM / ONE_D_RPM actions) or ADRP_ACT_PID / _VEL / _ONE_D_PID (fused DSLPIDControl);
// HELP (STG + auto-reset only): a second wave per block computes the next-episode initial state
// of the first wave's envs (3 Philox draws, quaternion, Euler obs: ~1/4 of a wave's instruction
// stream at E = 4096, where nearly every wave has a done lane) on another SIMD, into LDS; the
// chain wave, issue-bound at one instruction per 4 cycles, only copies it for its done lanes.
// SYS: the action rows live in host-mapped memory written by the host while the kernel runs
// (hover_persist.h): 1 = they are read with system-scope loads, which no GPU cache serves; 2 = the
// caller already read them (pre[0..A-1], the persistent kernel's line mode).
// FO: the state's field addressing (body_offsets): 1 = 32-bit offsets (the host saw that E fits), 0 = 64-bit
// indices, 2 = decided here from E (a branch at the loads and at the stores).
// What follows from those:
// ANG: the obs row's angles are computed by the helper waves from the chain's final quaternion (LDS): pitch
// and yaw by two more waves, the roll by the reset helper, whose own work ends before barrier A.  The chain's
// tail holds none of the three float64 atan2-class evaluations and ends at its state stores: the helper waves
// copy out all eighteen columns of the block (helper_ring, helper_tail).
// TW: the yaw helper is also the translation wave (PoseSlots)
// LATE_XY (ANG with unrolled sub-steps, no translation wave): pos.x / pos.y are summed behind barrier A
// (pyb_chain's vxy)
template <typename Real_, int PH_, int A_, int B_, int SC_, bool STG_, int CTL_, bool HELP_, int SYS_, int FO_>
struct StepForm {
    using Real = Real_;
    static constexpr int PH = PH_, A = A_, B = B_, SC = SC_, CTL = CTL_, SYS = SYS_, FO = FO_;
    static constexpr int BR = B > 0 ? B : 1;
    static constexpr bool STG = STG_, HELP = HELP_;
    static constexpr bool DRAG = (PH == ADRP_PHYS_PYB_DRAG || PH == ADRP_PHYS_PYB_GND_DRAG_DW);
    static constexpr bool DYN = (PH == ADRP_PHYS_DYN);
    static constexpr bool ANG = HELP && angle_helpers<Real>();
    static constexpr bool TW = ANG && PH == ADRP_PHYS_PYB && CTL == 0 && SC > 0;
    static constexpr bool LATE_XY = ANG && !DYN && SC > 0 && !TW;
    // the chain wave's share of the block's coalesced copy-out where it has one: every column without a
    // helper, half of them beside the single fp32 helper (ANG: none, the three helper waves copy out)
    static constexpr int kChainCols = HELP ? kRowF4 / 2 : kRowF4;
    static_assert(!HELP || STG, "the reset helper wave pairs with the staged (all lanes live) kernel");
    static_assert(!STG || (A == 4 && B == 15), "staged rows: 72-float rows only");
    using Lds = StepLds<Real, SC, STG, HELP, ANG, TW>;
};

// ---- pieces that more than one role runs ----

// BaseAviary.reset of a done lane from the reset helper's LDS copy
template <typename Real>
__device__ __forceinline__ void take_reset_state(const Real* rs_body, int t, Body<Real>& b, int32_t& sc, int32_t& ep) {
    Real v[kResetFields];
#pragma unroll
    for (int k = 0; k < kResetFields; ++k) v[k] = rs_body[k * kStepBlock + t];
    b.pos = v3(v[0], v[1], v[2]);
    b.q = {v[3], v[4], v[5], v[6]};
    b.ql = b.q;
    b.vel = v3(v[7], v[8], v[9]);
    b.w = v3(v[10], v[11], v[12]);
    b.angv = v3(v[13], v[14], v[15]);
#pragma unroll
    for (int i = 0; i < 4; ++i) b.prev_rpm[i] = Real(0);
    sc = 0;
    ep += 1;
}

// The ring part of a staged obs row, oldest first; the appended action av is the newest entry (deque.append).
// Every env appends once per env.step and resets keep the ring, so the head is the same for every env in
// practice: then the slot -> row position map is scalar and the action simply overwrites the newest position.
template <int B>
__device__ __forceinline__ void stage_ring(float4* my, const float (&rg)[B][4], float4 av, int32_t head) {
    const int hu = __builtin_amdgcn_readfirstlane(head);
    if (__all(head == hu)) {
        const int h1 = hu + 1 == B ? 0 : hu + 1;
#pragma unroll
        for (int p = 0; p < B; ++p) {
            const int k = p >= h1 ? p - h1 : p - h1 + B;
            my[3 + k] = make_float4(rg[p][0], rg[p][1], rg[p][2], rg[p][3]);
        }
        my[3 + B - 1] = av;
    } else {
        const int h1 = head + 1 == B ? 0 : head + 1;
#pragma unroll
        for (int p = 0; p < B; ++p) {
            int k = p - h1;
            k += k < 0 ? B : 0;
            const bool hit = p == head;
            my[3 + k] = make_float4(hit ? av.x : rg[p][0], hit ? av.y : rg[p][1], hit ? av.z : rg[p][2],
                                    hit ? av.w : rg[p][3]);
        }
    }
}

// reward, terminated and the position limits of truncated from a position (HoverAviary.py:68-117)
struct PosFlags {
    float rew;
    bool term, out;
};
template <typename Real>
__device__ __forceinline__ PosFlags hover_pos_flags(const HoverConst<Real>& C, V3<Real> pos) {
    const Real dx = C.target[0] - pos.x, dy = C.target[1] - pos.y, dz = C.target[2] - pos.z;
    const Real d2 = dx * dx + dy * dy + dz * dz;
    const Real r = Real(2) - d2 * d2;
    PosFlags f;
    f.rew = float(r > Real(0) ? r : Real(0));
    f.term = d2 < Real(1e-8);   // |target - pos| < 1e-4
    f.out = fabs_(pos.x) > Real(1.5) || fabs_(pos.y) > Real(1.5) || pos.z > Real(2.0);
    return f;
}

// ---- the ANG kernels' copy-out over the three helper waves (192 lanes) ----
//   before barrier C, while the chain is still at work, the fifteen ring columns, which are final at
//   barrier A: five float4 per lane (helper_ring);
//   behind barrier B the three kinematic columns, one float4 per lane (lane g: column g % 3 of row g / 3),
//   for a done env from the reset obs (kResetObs) instead of the staged row; and the staged rows of the
//   listed envs, which the reset never touches, as terminal rows, ten rows per pass over lanes 0..179
//   (lane g: list entry g / 18, column g % 18) (helper_tail).
constexpr int kHelpLanes = 3 * kStepBlock, kRingF4 = kRowF4 - 3;
constexpr int kRingPer = kStepBlock * kRingF4 / kHelpLanes;   // ring float4 per helper lane
constexpr int kTermRows = kHelpLanes / kRowF4;                // terminal rows per pass
static_assert(kRingPer * kHelpLanes == kStepBlock * kRingF4, "copy-out over three helper waves");
// What a helper lane's copies need that depends on the lane alone, formed (and held in registers) while
// the wave waits for barrier A.  Byte offsets within `rows`, which are the byte offsets within the block's
// obs rows too: ring[j] of ring float4 g + 192 j (column 3 + n % 15 of row n / 15), kin of the lane's
// kinematic float4, fix of the same column of the row's reset obs; flag: the row; sub, tcol: the lane's
// list entry and column of a terminal row pass
struct TailIdx {
    uint32_t ring[kRingPer], kin, fix, flag, sub, tcol;
};
__device__ __forceinline__ TailIdx tail_index(int tl, int wv) {
    TailIdx t;
    const uint32_t g = uint32_t(wv - 1) * kStepBlock + uint32_t(tl);
#pragma unroll
    for (int j = 0; j < kRingPer; ++j) {
        const uint32_t n = g + kHelpLanes * uint32_t(j);
        const uint32_t row = (n * 4370u) >> 16;   // n / 15 for n < 960
        t.ring[j] = (row * kRowF4 + 3u + (n - kRingF4 * row)) * 16u;
        asm volatile("" : "+v"(t.ring[j]));
    }
    t.flag = (g * 21846u) >> 16;                  // g / 3 for g < 192
    t.kin = (t.flag * kRowF4 + (g - 3u * t.flag)) * 16u;
    t.fix = (kResetObs + g) * 16u;
    t.sub = (g * 3641u) >> 16;                    // g / 18 for g < 192
    t.tcol = g - kRowF4 * t.sub;
    asm volatile("" : "+v"(t.kin), "+v"(t.fix), "+v"(t.flag), "+v"(t.sub), "+v"(t.tcol));
    return t;
}
__device__ __forceinline__ void helper_ring(const float4* rows, float* obs, const TailIdx& ti) {
    const char* lds = reinterpret_cast<const char*>(rows);
    char* dst = reinterpret_cast<char*>(obs) + size_t(blockIdx.x) * (kStepBlock * kRowF4 * sizeof(float4));
    float4 o[kRingPer];
#pragma unroll
    for (int j = 0; j < kRingPer; ++j) o[j] = *reinterpret_cast<const float4*>(lds + ti.ring[j]);
#pragma unroll
    for (int j = 0; j < kRingPer; ++j) store_out(reinterpret_cast<float4*>(dst + ti.ring[j]), o[j]);
}
// A helper lane's work behind barrier B.  The count, the first pass's list entry and, through it, the first
// pass's float4 are read ahead of the obs store, needed or not (a list entry past the count is stale: it
// is masked to a row of the block and not stored), so that the common single pass adds one predicated
// store to the wave's tail and no LDS round trip.
template <typename Real, typename Lds>
__device__ __forceinline__ void helper_tail(const HoverArgs<Real>& a, Lds& l, const TailIdx& ti) {
    const int cnt_v = l.done_cnt[0];
    const int row0 = l.done_list[ti.sub] & (kStepBlock - 1);
    const uint8_t fl = l.done_b[ti.flag];
    const char* lds = reinterpret_cast<const char*>(l.rows);
    char* dst = reinterpret_cast<char*>(a.obs) + size_t(blockIdx.x) * (kStepBlock * kRowF4 * sizeof(float4));
    const float4 o = *reinterpret_cast<const float4*>(lds + (fl ? ti.fix : ti.kin));
    float4 t0 = l.rows[row0 * kRowF4 + int(ti.tcol)];
    hold(t0.x); hold(t0.y); hold(t0.z); hold(t0.w);   // (the read stays here, ahead of the store)
    store_out(reinterpret_cast<float4*>(dst + ti.kin), o);
    const int cnt = __builtin_amdgcn_readfirstlane(cnt_v);
    const int sub = int(ti.sub), c = int(ti.tcol);
    const bool mine = sub < kTermRows;
    float4* tb = reinterpret_cast<float4*>(a.tobs) + size_t(blockIdx.x) * kStepBlock * kRowF4;
    if (mine && sub < cnt) tb[row0 * kRowF4 + c] = t0;
    for (int base = kTermRows; base < cnt && base < kStepBlock; base += kTermRows) {
        const int n = base + sub;
        if (mine && n < cnt) {
            const int row = l.done_list[n] & (kStepBlock - 1);
            tb[row * kRowF4 + c] = l.rows[row * kRowF4 + c];
        }
    }
}

// ---- role: the translation wave (wave 3 of a TW kernel; PoseSlots has the protocol) ----
// It loads pos, vel, the two quaternions of slots 0 and 1 and the action itself, forms the prop force sum
// as pyb_chain does, and per sub-step s polls the mark of its thrust axis and runs pyb_trans_substep; only
// when a lane is near the plane does it also wait for slot s + 2 (the pose behind the sub-step) for the
// contact test.  It owns the contact counter, the reward, `terminated`, the position limits of `truncated`
// (tw_flag) and row floats 0-2 and 6-8, and leaves the final pos / vel in tw_out.  Every state store stays
// on the chain.
template <typename Real>
struct TransWave {
    V3<Real> pos{}, vel{};
    Q4<Real> q{}, ql{};   // slots 1 and 0 of the hand-off: what the chain loads as b.q and b.ql
    float4 act = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float rew = 0.0f;
    bool term = false;
};
// its loads first, the marks cleared (and the clears landed) before the head barrier
template <class F>
__device__ __forceinline__ void trans_wave_load(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                                typename F::Lds& l, int tl, TransWave<typename F::Real>& t) {
    using Real = typename F::Real;
    const int te_ = int(blockIdx.x) * kStepBlock + tl;
    auto fld = [&](int k) {
        if constexpr (F::FO == 1) return field_at(a.f, (uint32_t(k) * uint32_t(a.E) + uint32_t(te_)) * uint32_t(sizeof(Real)));
        else return a.f[size_t(k) * a.E + te_];
    };
    t.pos = v3(fld(HF_POS + 0), fld(HF_POS + 1), fld(HF_POS + 2));
    t.vel = v3(fld(HF_VEL + 0), fld(HF_VEL + 1), fld(HF_VEL + 2));
    t.q = {fld(HF_QUAT + 0), fld(HF_QUAT + 1), fld(HF_QUAT + 2), fld(HF_QUAT + 3)};
    t.ql = t.q;
    if (C.link_lag)
        t.ql = {fld(HF_LINK_QUAT + 0), fld(HF_LINK_QUAT + 1), fld(HF_LINK_QUAT + 2), fld(HF_LINK_QUAT + 3)};
    t.act = reinterpret_cast<const float4*>(a.act)[te_];
    l.slots().clear(tl);
}
// the translational half of the sub-steps, behind the chain's poses; reward and flags
template <class F>
__device__ __forceinline__ void hover_trans_wave(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                                 typename F::Lds& l, int tl, TransWave<typename F::Real>& t) {
    using Real = typename F::Real;
    const auto slots = l.slots();
    const bool lag = C.link_lag;
    ChainK<Real> K = chain_consts<Real>();
    HoverConst<Real> Cp = C;
    pin(K.k004); pin(K.c100); pin(K.nn_min);
    pin(Cp.dt); pin(Cp.mass); pin(Cp.gravity); pin(Cp.inv_mass);
    pin(Cp.coll_hh); pin(Cp.coll_r); pin(Cp.coll_zoff);
    const float ta[4] = {t.act.x, t.act.y, t.act.z, t.act.w};
    Real rpm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rpm[i] = C.hover_rpm * Real(rpm_gain(ta[i]));
    const Real sum_f = prop_sums(C, rpm).sum_f;
    bool touched = false;
    [[maybe_unused]] bool near = false;
#pragma unroll
    for (int s = 0; s < F::SC; ++s) {
        const int k = lag ? s : s + 1;
        V3<Real> zs;
        if (k < 2) {
            zs = col2_fm(k == 0 ? t.ql : t.q);
        } else {
            slots.wait(k);
            zs = slots.zaxis(k, tl);
        }
        pyb_trans_substep(Cp, t.pos, t.vel, zs, sum_f, K);
        if (pyb_trans_near_plane(Cp, t.pos)) {   // (rare) the pose behind this sub-step
            slots.wait(s + 2);
            touched |= pyb_trans_contact(Cp, t.pos, t.vel, slots.zaxis(s + 2, tl));
            near = true;
        }
    }
    if (touched && a.contact_count) atomicAdd(a.contact_count, 1);
#ifdef ADRP_RACE_TIMING
    if (tl == 0 && near) atomicAdd(&g_race_phase[24], 1ull);   // waves that took the near-plane path
#endif
    // the chain adds the step limit and the tilt to the flag byte's second bit
    const PosFlags pf = hover_pos_flags(C, t.pos);
    t.rew = pf.rew;
    t.term = pf.term;
    l.tw_out[(HF_POS + 0) * kStepBlock + tl] = t.pos.x; l.tw_out[(HF_POS + 1) * kStepBlock + tl] = t.pos.y;
    l.tw_out[(HF_POS + 2) * kStepBlock + tl] = t.pos.z;
    l.tw_out[(HF_VEL + 0) * kStepBlock + tl] = t.vel.x; l.tw_out[(HF_VEL + 1) * kStepBlock + tl] = t.vel.y;
    l.tw_out[(HF_VEL + 2) * kStepBlock + tl] = t.vel.z;
    l.tw_flag[tl] = uint8_t((pf.term ? 1 : 0) | (pf.out ? 2 : 0));
#ifdef ADRP_RACE_TIMING
    if (tl == 0) l.tw_time[0] = __builtin_amdgcn_s_memtime();   // this wave's arrival at A
#endif
}
// what of the translation the chain does not wait for: behind A, where this wave has slack
template <typename Real>
__device__ __forceinline__ void trans_wave_rows(const HoverArgs<Real>& a, float* rowf, int tl, const TransWave<Real>& t) {
    const int te_ = int(blockIdx.x) * kStepBlock + tl;
    a.rew[te_] = t.rew;
    a.term[te_] = t.term;
    rowf[0] = float(t.pos.x); rowf[1] = float(t.pos.y); rowf[2] = float(t.pos.z);
    rowf[6] = float(t.vel.x); rowf[7] = float(t.vel.y); rowf[8] = float(t.vel.z);
}

// ---- role: the angle helpers (ANG kernels): pitch (wave 2), yaw (wave 3, in TW kernels behind the translation) ----
template <class F>
__device__ __forceinline__ void hover_angle_helper(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                                   typename F::Lds& l) {
    using Real = typename F::Real;
    const int tl = threadIdx.x & (kStepBlock - 1), wv = threadIdx.x / kStepBlock;
    [[maybe_unused]] const bool trans = F::TW && __builtin_amdgcn_readfirstlane(wv) == 3;
    [[maybe_unused]] TransWave<Real> tw;
    if constexpr (F::TW) {
        if (trans) trans_wave_load<F>(a, C, l, tl, tw);
        F::Lds::Slots::head();
    }
    AngK ak = ang_consts();   // the lean angle forms' constants, into VGPRs while the wave is idle
    pin_all(ak);
    const TailIdx ti = tail_index(tl, wv);
    if constexpr (F::TW) {
        if (trans) hover_trans_wave<F>(a, C, l, tl, tw);
    }
    __syncthreads();   // A: the chain's final quaternion
    const Q4<Real> q = l.ang_q_read(tl);
    float* rowf = reinterpret_cast<float*>(l.rows) + tl * (4 * kRowF4);
    if constexpr (F::TW) {
        if (trans) trans_wave_rows(a, rowf, tl, tw);
    }
    if (wv == 2) {
        const double p = euler_pitch_lean(q, ak);
        l.ang_p[tl] = p;
        rowf[4] = float(p);
    } else {
        const float y = float(euler_yaw_lean(q, ak));
        l.ang_y[tl] = y;
        rowf[5] = y;
    }
    helper_ring(l.rows, a.obs, ti);
    __syncthreads();   // C: pitch and yaw
    __syncthreads();   // B: the final rows
    helper_tail(a, l, ti);
}

// ---- role: the reset-and-ring helper (wave 1 of a HELP kernel) ----
// The action ring's part of the obs row is independent of the physics, so this wave loads it, stages it in LDS
// and appends the action; it draws the next-episode state of every env of the block and its obs into LDS; and
// in ANG kernels, idle from barrier A to the copy-out, it takes the roll.
template <class F>
__device__ __forceinline__ void hover_reset_helper(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                                   typename F::Lds& l) {
    using Real = typename F::Real;
    constexpr int B = F::B;
    const int tl = threadIdx.x - kStepBlock;
    const int he = blockIdx.x * kStepBlock + tl;
    const int E = a.E;
    if constexpr (F::TW) F::Lds::Slots::head();   // (the translation wave's marks are clear)
    const float4 av = reinterpret_cast<const float4*>(a.act)[he];
    float rg[B][4];    // plain floats: float4 struct copies under a select went to scratch
#pragma unroll
    for (int p = 0; p < B; ++p) {
        const float4 v = reinterpret_cast<const float4*>(a.ring)[size_t(p) * E + he];
        rg[p][0] = v.x; rg[p][1] = v.y; rg[p][2] = v.z; rg[p][3] = v.w;
    }
    const int32_t head = a.ist[HI_RING_HEAD * E + he];
    int32_t hsc = 0, hep = a.ist[HI_EPISODE * E + he];
    Body<Real> rb;
    hover_reset_state(a, C, he, rb, hsc, hep);
    float o[12];
    hover_obs12(C, rb, o);
    const Real v[kResetFields] = {rb.pos.x, rb.pos.y, rb.pos.z, rb.q.x, rb.q.y, rb.q.z, rb.q.w,
                                  rb.vel.x, rb.vel.y, rb.vel.z, rb.w.x, rb.w.y, rb.w.z,
                                  rb.angv.x, rb.angv.y, rb.angv.z};
#pragma unroll
    for (int k = 0; k < kResetFields; ++k) l.rs_body[k * kStepBlock + tl] = v[k];
    if constexpr (F::ANG) {   // as three float4: the helper waves' copy-out takes them whole (helper_tail)
        l.rows[kResetObs + 3 * tl + 0] = make_float4(o[0], o[1], o[2], o[3]);
        l.rows[kResetObs + 3 * tl + 1] = make_float4(o[4], o[5], o[6], o[7]);
        l.rows[kResetObs + 3 * tl + 2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) l.rs_obs[k * kStepBlock + tl] = o[k];
    }
    stage_ring<B>(l.rows + tl * kRowF4, rg, av, head);
    reinterpret_cast<float4*>(a.ring)[size_t(head) * E + he] = av;
    if constexpr (F::ANG) {
        AngK ak = ang_consts();   // (pinned behind this wave's reset work, before A)
        pin_all(ak);
        const TailIdx ti = tail_index(tl, 1);
        __syncthreads();   // A: reset states and ring rows in LDS; the chain's final quaternion
        const double roll = euler_roll_lean(l.ang_q_read(tl), ak);
        l.ang_r[tl] = roll;
        reinterpret_cast<float*>(l.rows)[tl * (4 * kRowF4) + 3] = float(roll);
        helper_ring(l.rows, a.obs, ti);
        __syncthreads();   // C: the roll
        __syncthreads();   // B: the chain wave's done marks
        helper_tail(a, l, ti);
    } else {
        __syncthreads();   // A: reset states and ring rows in LDS
        __syncthreads();   // B: the chain wave's kinematic parts
        // this wave's part of the block's coalesced copy-out
        float4* dst = reinterpret_cast<float4*>(a.obs) + size_t(blockIdx.x) * kStepBlock * kRowF4;
#pragma unroll
        for (int k = F::kChainCols; k < kRowF4; ++k) store_out(dst + tl + kStepBlock * k, l.rows[tl + kStepBlock * k]);
    }
}

// ---- role: the chain wave; also the whole step of the kernels without helpers and of the persistent kernel ----
// one lane's env through the step: where its state lies, the state, the action and (without a helper) the ring
template <class F>
struct ChainLane {
    using Real = typename F::Real;
    int e, D;
    bool split, lag, fit;
    BodyOffs<Real> fo;    // one 32-bit byte offset per field on the uniform base (body_offsets), kept for the stores
    uint32_t io[HI_N];
    Body<Real> b;
    int32_t sc, ep, head, head1;
    float act[F::A];
    float ring[F::BR][F::A];
};
// ---- issue every load up front: state (the chain's first operands) and ints, action, the whole ring ----
template <class F>
__device__ __forceinline__ void chain_loads(const HoverArgs<typename F::Real>& a, const float* pre, ChainLane<F>& L) {
    using Real = typename F::Real;
    constexpr int A = F::A, B = F::B;
    const int E = a.E, e = L.e;
    // (the offsets are formed on both sides of the branch, so that they are no merged values at the stores)
    L.fo = body_offsets<Real>(E, e, L.lag, F::DRAG, F::DYN);
    field_run(uint32_t(e) * 4u, uint32_t(E) * 4u, 0, HI_N, L.io);
    int32_t head_ld;
    if (L.fit) {
        load_body_at<Real>(a.f, L.fo, L.b, L.lag, F::DRAG, F::DYN, !F::TW);
        L.sc = field_at(a.ist, L.io[HI_STEP]); L.ep = field_at(a.ist, L.io[HI_EPISODE]); head_ld = field_at(a.ist, L.io[HI_RING_HEAD]);
        field_form_end();
    } else {
        load_body(a, e, L.b, L.lag, F::DRAG, F::DYN);
        L.sc = a.ist[HI_STEP * E + e]; L.ep = a.ist[HI_EPISODE * E + e]; head_ld = a.ist[HI_RING_HEAD * E + e];
        if constexpr (F::TW) L.b.pos = L.b.vel = v3(Real(0), Real(0), Real(0));   // (the translation wave's: these loads are dead)
    }
    L.head = head_ld;
    if constexpr (F::SYS == 2) {
#pragma unroll
        for (int j = 0; j < A; ++j) L.act[j] = pre[j];
    } else if constexpr (F::SYS == 1) {
        uint32_t* sa = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(a.act)) + size_t(e) * A;
#pragma unroll
        for (int j = 0; j < A; ++j)
            L.act[j] = __uint_as_float(__hip_atomic_load(sa + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    } else if constexpr (A == 4) {
        const float4 v = reinterpret_cast<const float4*>(a.act)[e];
        L.act[0] = v.x; L.act[1] = v.y; L.act[2] = v.z; L.act[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < A; ++j) L.act[j] = a.act[e * A + j];
    }
#pragma unroll
    for (int p = 0; p < (F::HELP ? 0 : B); ++p) {   // (no-op for B == 0; HELP: the helper wave's job)
        if constexpr (A == 4) {
            const float4 v = reinterpret_cast<const float4*>(a.ring)[size_t(p) * E + e];
            L.ring[p][0] = v.x; L.ring[p][1] = v.y; L.ring[p][2] = v.z; L.ring[p][3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < A; ++j) L.ring[p][j] = a.ring[(size_t(p) * E + e) * A + j];
        }
    }
}
// ---- _preprocessAction: RPM = HOVER_RPM * (1 + 0.05 a), the gain in float32 (NEP 50),
//      or the DSLPIDControl output for the PID action types ----
template <class F>
__device__ __forceinline__ void chain_rpm(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                          const ChainLane<F>& L, typename F::Real rpm[4]) {
    using Real = typename F::Real;
    constexpr int A = F::A, CTL = F::CTL;
    if constexpr (CTL != 0) {
        static_assert(A == (CTL == ADRP_ACT_PID ? 3 : CTL == ADRP_ACT_VEL ? 4 : 1), "PID action width");
        const int E = a.E, e = L.e;
        Real ctl[HF_NPID];
        uint32_t po[HF_PID + HF_NPID];
        field_run(uint32_t(e) * uint32_t(sizeof(Real)), uint32_t(E) * uint32_t(sizeof(Real)), HF_PID, HF_NPID, po);
        if (L.fit) {
#pragma unroll
            for (int k = 0; k < HF_NPID; ++k) ctl[k] = field_at(a.f, po[HF_PID + k]);
            field_form_end();
        } else {
#pragma unroll
            for (int k = 0; k < HF_NPID; ++k) ctl[k] = a.f[(HF_PID + k) * E + e];
        }
        dslpid_rpm<Real, CTL>(C, L.b, L.act, ctl, rpm);
        if (L.fit) {
#pragma unroll
            for (int k = 0; k < HF_NPID; ++k) field_last(a.f, po[HF_PID + k]) = ctl[k];
            field_form_end();
        } else {
#pragma unroll
            for (int k = 0; k < HF_NPID; ++k) a.f[(HF_PID + k) * E + e] = ctl[k];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) rpm[i] = C.hover_rpm * Real(rpm_gain(L.act[A == 1 ? 0 : i]));
    }
}
// the state and the ints leave through the offsets of the loads
template <class F>
__device__ __forceinline__ void chain_store_state(const HoverArgs<typename F::Real>& a, ChainLane<F>& L) {
    using Real = typename F::Real;
    const int E = a.E, e = L.e;
    if (L.fit) {
        store_body_at<Real>(a.f, L.fo, L.b, L.lag, F::DRAG, F::DYN);
        field_last(a.ist, L.io[HI_STEP]) = L.sc;
        field_last(a.ist, L.io[HI_EPISODE]) = L.ep;
        field_last(a.ist, L.io[HI_RING_HEAD]) = L.head1;
        field_form_end();
    } else {
        store_body(a, e, L.b, L.lag, F::DRAG, F::DYN);
        a.ist[HI_STEP * E + e] = L.sc;
        a.ist[HI_EPISODE * E + e] = L.ep;
        a.ist[HI_RING_HEAD * E + e] = L.head1;
    }
}
// ANG, behind the final quaternion: barrier A, and the chain's part of the obs row.
// While the three helper waves take one angle each, the chain does what only it can: ω back to the world
// frame (deferred by pyb_chain), the conversions and, in the caller, the reward and the angle-free truncation
// tests.  (hold: arithmetic carries no order against a barrier, and the compiler had placed most of this
// before A and the rest after C, leaving the chain to wait at C with nothing to do; what the work starts from
// is taken behind A here, and what it gives is finished before C in the caller.)
template <class F>
__device__ __forceinline__ void chain_row_behind_A(const HoverConst<typename F::Real>& C, typename F::Lds& l, Body<typename F::Real>& b,
                                                   V3<typename F::Real>& wbf, typename F::Real* vxy, float o12[12]) {
    using Real = typename F::Real;
    constexpr bool TW = F::TW;
    l.ang_q_write(threadIdx.x, b.q);
#ifdef ADRP_RACE_TIMING
    [[maybe_unused]] const uint64_t t_a = __builtin_amdgcn_s_memtime();   // the chain's arrival at A
#endif
    __syncthreads();   // A: the quaternion out; the reset helper's states and ring rows in
#ifdef ADRP_RACE_TIMING
    if constexpr (TW) {   // [20] / [21]: cycles the translation wave arrived at A before / behind the chain
        if (threadIdx.x == 0) {
            const uint64_t t_w = l.tw_time[0];
            atomicAdd(&g_race_phase[t_a >= t_w ? 20 : 21], (unsigned long long)(t_a >= t_w ? t_a - t_w : t_w - t_a));
        }
    }
#endif
    if constexpr (TW) {   // the translation wave's final pos / vel, read while the chain has arithmetic to do
        const Real* src = l.tw_out + threadIdx.x;
        b.pos = v3(src[(HF_POS + 0) * kStepBlock], src[(HF_POS + 1) * kStepBlock], src[(HF_POS + 2) * kStepBlock]);
        b.vel = v3(src[(HF_VEL + 0) * kStepBlock], src[(HF_VEL + 1) * kStepBlock], src[(HF_VEL + 2) * kStepBlock]);
    }
    hold(b.q.x); hold(b.q.y); hold(b.q.z); hold(b.q.w);
    hold(wbf.x); hold(wbf.y); hold(wbf.z);
    if constexpr (!TW) { hold(b.pos.x); hold(b.pos.y); hold(b.pos.z); }
    if constexpr (F::LATE_XY) {   // the horizontal position sums of the sub-steps, deferred to here
#pragma unroll
        for (int k = 0; k < 2 * F::SC; ++k) hold(vxy[k]);
#pragma unroll
        for (int s = 0; s < F::SC; ++s) {
            b.pos.x = fmx(C.dt, vxy[2 * s], b.pos.x);
            b.pos.y = fmx(C.dt, vxy[2 * s + 1], b.pos.y);
        }
    }
    if constexpr (!TW) { hold(b.vel.x); hold(b.vel.y); hold(b.vel.z); }
    if constexpr (!F::DYN) b.w = mul(rot_fm(b.q), wbf);
    const V3<Real> w = C.physics == ADRP_PHYS_DYN ? b.angv : b.w;   // hover_obs12's row, the angles are the helpers'
    if constexpr (!TW) {   // (TW: row floats 0-2 and 6-8 are the translation wave's)
        o12[0] = float(b.pos.x); o12[1] = float(b.pos.y); o12[2] = float(b.pos.z);
        o12[6] = float(b.vel.x); o12[7] = float(b.vel.y); o12[8] = float(b.vel.z);
    }
    o12[9] = float(w.x);     o12[10] = float(w.y);    o12[11] = float(w.z);
}
// The chain's end in ANG kernels: its nine floats of the row that are not angles (the helper waves write
// floats 3, 4, 5; TW: three, the translation wave has the other six), one byte per lane (done_b: the env is
// done), the done lanes into done_list at their rank and the count into done_cnt for the helper waves' tail,
// the reset state of its done lanes from rs_body, the state stores, barriers C and B.
template <class F>
__device__ __forceinline__ void chain_end_helpers(const HoverArgs<typename F::Real>& a, typename F::Lds& l, ChainLane<F>& L,
                                                  const float o12[12], bool done, bool slow, [[maybe_unused]] uint64_t& t4) {
    float4* my = l.rows + threadIdx.x * kRowF4;
    float* mf = reinterpret_cast<float*>(my);
    if constexpr (F::TW) {
        mf[9] = o12[9]; mf[10] = o12[10]; mf[11] = o12[11];
    } else {
        mf[0] = o12[0]; mf[1] = o12[1]; mf[2] = o12[2];
        mf[6] = o12[6]; mf[7] = o12[7];
        my[2] = make_float4(o12[8], o12[9], o12[10], o12[11]);
    }
    const unsigned long long done_mask = __ballot(done);
    l.done_b[threadIdx.x] = done;
    l.done_cnt[0] = a.tobs ? __popcll(done_mask) : 0;   // (every lane writes the same word)
    if (done) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(done_mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(done_mask), 0u));
        l.done_list[rank] = uint8_t(threadIdx.x);
        take_reset_state(l.rs_body, threadIdx.x, L.b, L.sc, L.ep);
    }
    RACE_SET(t4);
    chain_store_state(a, L);
    if (!slow) __syncthreads();   // C (the unsure wave passed it above)
    __syncthreads();              // B: the helper waves copy out
}
// The chain's end in the other staged kernels.  The obs row is assembled in LDS (18 float4 per lane, no
// padding: the copy-out reads contiguous float4s at immediate offsets) and leaves as one coalesced block.
template <class F>
__device__ __forceinline__ void chain_end_staged(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                                 typename F::Lds& l, ChainLane<F>& L, float o12[12], bool done,
                                                 [[maybe_unused]] uint64_t& t4) {
    float4* my = l.rows + threadIdx.x * kRowF4;
    // (HELP: the ring part of the row is staged by the helper wave)
    if constexpr (!F::HELP) stage_ring<F::B>(my, L.ring, make_float4(L.act[0], L.act[1], L.act[2], L.act[3]), L.head);
    my[0] = make_float4(o12[0], o12[1], o12[2], o12[3]);
    my[1] = make_float4(o12[4], o12[5], o12[6], o12[7]);
    my[2] = make_float4(o12[8], o12[9], o12[10], o12[11]);
    if constexpr (F::HELP) __syncthreads();   // A: the helper wave's reset states
    if (done) {
        if (a.tobs) {   // terminal obs = the row just staged (this lane's own LDS row)
            float4 t[kRowF4];
#pragma unroll
            for (int k = 0; k < kRowF4; ++k) t[k] = my[k];
            float4* trow = reinterpret_cast<float4*>(a.tobs + size_t(L.e) * L.D);
#pragma unroll
            for (int k = 0; k < kRowF4; ++k) trow[k] = t[k];
        }
        if constexpr (F::HELP) {
            const int t = threadIdx.x;
            take_reset_state(l.rs_body, t, L.b, L.sc, L.ep);
#pragma unroll
            for (int k = 0; k < 12; ++k) o12[k] = l.rs_obs[k * kStepBlock + t];
        } else {
            hover_reset_state(a, C, L.e, L.b, L.sc, L.ep);
            hover_obs12(C, L.b, o12);      // the reset keeps the ring: only the kinematic part changes
        }
        my[0] = make_float4(o12[0], o12[1], o12[2], o12[3]);
        my[1] = make_float4(o12[4], o12[5], o12[6], o12[7]);
        my[2] = make_float4(o12[8], o12[9], o12[10], o12[11]);
    }
    RACE_SET(t4);
    // the state leaves first: its registers are free before the copy-out (holding both
    // spilled the copy-out buffer to scratch)
    chain_store_state(a, L);
    __syncthreads();   // B (without a helper: the block's rows)
    float4* dst = reinterpret_cast<float4*>(a.obs) + size_t(blockIdx.x) * kStepBlock * kRowF4;
#pragma unroll
    for (int k = 0; k < F::kChainCols; ++k) store_out(dst + threadIdx.x + kStepBlock * k, l.rows[threadIdx.x + kStepBlock * k]);
}
// The chain's end in the row-store kernels: 16-byte stores per lane straight from registers
template <class F>
__device__ __forceinline__ void chain_end_rows(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                               ChainLane<F>& L, float o12[12], bool done, [[maybe_unused]] uint64_t& t4) {
    constexpr int A = F::A, B = F::B;
    const int E = a.E, e = L.e, D = L.D;
#pragma unroll
    for (int p = 0; p < B; ++p) {
        const bool hit = p == L.head;
#pragma unroll
        for (int j = 0; j < A; ++j) L.ring[p][j] = hit ? L.act[j] : L.ring[p][j];
    }
    if (done) {
        if (a.tobs) {
            if constexpr (B > 0) write_row<A, B>(a.tobs + size_t(e) * D, o12, L.ring, L.head1);
            else write_row_generic<A>(a.tobs + size_t(e) * D, o12, a.ring, a.B, E, e, L.head1, L.act, true);
        }
        hover_reset_state(a, C, e, L.b, L.sc, L.ep);
        if (L.split) hover_obs12_split(C, L.b, o12);
        else hover_obs12(C, L.b, o12);
    }
    RACE_SET(t4);
    if constexpr (B > 0) write_row<A, B>(a.obs + size_t(e) * D, o12, L.ring, L.head1);
    else write_row_generic<A>(a.obs + size_t(e) * D, o12, a.ring, a.B, E, e, L.head1, L.act, true);
}

template <class F>
__device__ __forceinline__ void hover_chain_wave(const HoverArgs<typename F::Real>& a, const HoverConst<typename F::Real>& C,
                                                 typename F::Lds& l, const float* pre) {
    using Real = typename F::Real;
    constexpr int A = F::A, B = F::B, SC = F::SC;
    constexpr bool STG = F::STG, HELP = F::HELP, ANG = F::ANG, TW = F::TW, DRAG = F::DRAG, DYN = F::DYN, LATE_XY = F::LATE_XY;
    const int E = a.E;
    ChainLane<F> L;
    // SPLIT (a step of ONE env, BASELINE config 1: launched or persistent): every lane of the wave runs
    // env 0 (the same inputs, the same code: the duplicate stores write the same values) so that three
    // lanes can take the three obs angles at once; contacts are counted by lane 0 alone
    L.split = !STG && !HELP && E == 1;
    L.e = L.split ? 0 : int(blockIdx.x) * kStepBlock + int(threadIdx.x);
    L.D = B > 0 ? 12 + B * A : a.D;
    if (L.e >= E) return;
    const int e = L.e;
    RACE_MARK(t0);
    L.fit = F::FO == 2 ? field_offsets_fit<Real>(E) : F::FO == 1;
    L.lag = C.link_lag && !DYN;
    chain_loads<F>(a, pre, L);
    Real rpm[4];
    chain_rpm<F>(a, C, L, rpm);
    Body<Real>& b = L.b;
    // ---- sub-step loop (BaseAviary.py:347-376) ----
    bool touched = false;
    V3<Real> wbf = v3(Real(0), Real(0), Real(0));   // ANG: the chain's final ω, still in the body frame
    Real vxy[LATE_XY ? 2 * SC : 2] = {};
#ifdef ADRP_RACE_TIMING
    // loads landed: the rpm gains and the state are consumed by the first sub-step
    __builtin_amdgcn_s_waitcnt(0);
#endif
    RACE_MARK(t1);
    if constexpr (DYN) {
        if constexpr (SC > 0) {
#pragma unroll
            for (int s = 0; s < SC; ++s) dyn_substep(C, b, rpm);
        } else {
            for (int s = 0; s < C.S; ++s) dyn_substep(C, b, rpm);
        }
    } else if constexpr (TW) {   // the rotational half; the poses go to the translation wave
        pyb_chain<Real, F::PH, SC, DRAG>(C, b, rpm, L.lag, NoExtForce{}, &wbf, nullptr, l.slots());
    } else {
        touched = pyb_chain<Real, F::PH, SC, DRAG>(C, b, rpm, L.lag, NoExtForce{}, ANG ? &wbf : nullptr, LATE_XY ? vxy : nullptr);
    }
    RACE_MARK(t2);
    if (touched && a.contact_count && (!L.split || threadIdx.x == 0)) atomicAdd(a.contact_count, 1);
    // ---- action ring: append this action at `head` (deque.append, BaseRLAviary.py:187) ----
    if constexpr (HELP) {
        // the helper wave appends
    } else if constexpr (A == 4)
        reinterpret_cast<float4*>(a.ring)[size_t(L.head) * E + e] = make_float4(L.act[0], L.act[1], L.act[2], L.act[3]);
    else
#pragma unroll
        for (int j = 0; j < A; ++j) a.ring[(size_t(L.head) * E + e) * A + j] = L.act[j];
    const int BB = B > 0 ? B : a.B;                    // ring length (runtime for the generic kernel)
    L.head1 = L.head + 1 == BB ? 0 : L.head + 1;
    // ---- obs / reward / terminated / truncated (HoverAviary.py:68-117) ----
    float o12[12];
    V3<Real> rpy;
    if constexpr (ANG) chain_row_behind_A<F>(C, l, b, wbf, vxy, o12);
    else if (L.split) rpy = hover_obs12_split(C, b, o12);
    else rpy = hover_obs12(C, b, o12);
    bool te, tr;
    if constexpr (TW) {   // the translation wave's flag byte
        const uint8_t fl = l.tw_flag[threadIdx.x];
        te = (fl & 1) != 0;
        tr = (fl & 2) != 0 || L.sc >= C.trunc_steps;
    } else {
        const PosFlags pf = hover_pos_flags(C, b.pos);
        a.rew[e] = pf.rew;
        te = pf.term;
        tr = pf.out || L.sc >= C.trunc_steps;
    }
    [[maybe_unused]] bool slow = false;   // ANG: the chain has waited at C for the angles
    if constexpr (ANG) {
        hold(b.w.x); hold(b.w.y); hold(b.w.z);
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (TW ? k > 8 : (k < 3 || k > 5)) hold(o12[k]);
        // The tilt truncation without waiting for an angle (trunc_from_quat).  One unsure lane sends the whole
        // wave down the path of before: wait at C for the helpers' roll and pitch and test those, so every
        // input gives the flag it gave.  Either way the wave passes A, C and B once each: on the sure path C
        // comes behind the state stores, next to B (slow is wave-uniform)
        TruncK tk = trunc_consts();
        pin_all(tk);
        bool over = false;
        const bool sure = trunc_from_quat(b.q, tk, over);
        slow = __any(!sure);
        if (__builtin_expect(slow, 0)) {
            __syncthreads();   // C: the helpers' roll and pitch
            rpy.x = l.ang_r[threadIdx.x];
            rpy.y = l.ang_p[threadIdx.x];
            over = fabs_(rpy.x) > Real(0.4) || fabs_(rpy.y) > Real(0.4);
        }
        tr = tr || over;
    } else {
        tr = tr || fabs_(rpy.x) > Real(0.4) || fabs_(rpy.y) > Real(0.4);
    }
    if constexpr (!TW) a.term[e] = te;
    a.trunc[e] = tr;
    L.sc += C.S;
    const bool done = a.autoreset && (te || tr);
    RACE_MARK(t3);
#ifdef ADRP_RACE_TIMING
    const unsigned long long dmask = __ballot(done);
#endif
    [[maybe_unused]] uint64_t t4 = 0;
    if constexpr (ANG) chain_end_helpers<F>(a, l, L, o12, done, slow, t4);
    else if constexpr (STG) chain_end_staged<F>(a, C, l, L, o12, done, t4);
    else chain_end_rows<F>(a, C, L, o12, done, t4);
    RACE_MARK(t5);
    if constexpr (!STG) chain_store_state(a, L);
#ifdef ADRP_RACE_TIMING
    RACE_MARK(t6);
    if (threadIdx.x == 0) {   // [loads, sub-steps, obs+flags, reset, obs row, state stores, total, -, waves]
        RACE_ACC(0, t1 - t0); RACE_ACC(1, t2 - t1); RACE_ACC(2, t3 - t2); RACE_ACC(3, t4 - t3);
        RACE_ACC(4, t5 - t4); RACE_ACC(5, t6 - t5); RACE_ACC(6, t6 - t0); RACE_ACC(8, 1);
        RACE_ACC(7, __popcll(dmask));
        if (dmask) atomicAdd(&g_race_phase[9], 1ull);
    }
#endif
}

// The step: the workgroup's LDS and one role per wave.  Who passes which barrier, once each, behind what:
//            chain wave (0)                      reset helper (1, HELP)          angle helpers (2 and 3, ANG)
//   head     pyb_chain's pre-loop, ahead of      its entry                       wave 3's loads and mark clears
//   (TW)     the first pose (hand.head())
//   A        its final quaternion in LDS;        reset states, ring rows and     wave 3: the translation's
//   (HELP)   fp32: its kinematic row floats      the ring append                 pos / vel / flags in LDS
//   C        sure tilt: its state stores;        the roll, its ring columns      pitch (2), yaw (3), their
//   (ANG)    unsure: ahead of reading roll                                       ring columns
//            and pitch, then the state stores
//   B        C, or fp32 its state stores         C, or fp32 A                    C
//   then     fp32: columns 0-8 out; ANG: ends    fp32: columns 9-17 out; ANG:    helper_tail
//                                                helper_tail
template <typename Real, int PH, int A, int B, int SC, bool STG = false, int CTL = 0, bool HELP = false, int SYS = 0,
          int FO = 2>
__device__ __forceinline__ void hover_step_body(const HoverArgs<Real>& a, const HoverConst<Real>& C,
                                                const float* pre = nullptr) {
    using F = StepForm<Real, PH, A, B, SC, STG, CTL, HELP, SYS, FO>;
    using Lds = typename F::Lds;
    constexpr bool ANG = F::ANG, TW = F::TW;
    constexpr int kLane = kStepBlock;   // (an array the kernel does not have is one element that nothing names)
    __shared__ float4 rows[Lds::kRows];
    __shared__ typename Lds::Slots::Real2 tw_q[TW ? 2 * SC * kLane : 1];
    __shared__ Real rs_body[HELP ? kResetFields * kLane : 1], tw_out[TW ? Lds::kTwOut * kLane : 1];
    __shared__ Real ang_q_own[ANG && !TW ? 4 * kLane : 1], ang_r[ANG ? kLane : 1], ang_p[ANG ? kLane : 1];
    __shared__ float rs_obs[HELP && !ANG ? 12 * kLane : 1], ang_y[ANG ? kLane : 1];
    __shared__ int done_cnt[1], tw_mark[TW ? Lds::Slots::kSlots : 1];
    __shared__ uint8_t done_list[ANG ? kLane : 1], done_b[ANG ? kLane : 1], tw_flag[TW ? kLane : 1];
#ifdef ADRP_RACE_TIMING
    __shared__ unsigned long long tw_time[1];
    Lds lds = {rows, tw_q, rs_body, tw_out, ang_q_own, ang_r, ang_p, rs_obs, ang_y, done_cnt, tw_mark, done_list, done_b,
               tw_flag, tw_time};
#else
    Lds lds = {rows, tw_q, rs_body, tw_out, ang_q_own, ang_r, ang_p, rs_obs, ang_y, done_cnt, tw_mark, done_list, done_b,
               tw_flag};
#endif
    if constexpr (F::ANG) {
        if (threadIdx.x >= 2 * kStepBlock) return hover_angle_helper<F>(a, C, lds);
    }
    if constexpr (HELP) {
        if (threadIdx.x >= kStepBlock) return hover_reset_helper<F>(a, C, lds);
    }
    hover_chain_wave<F>(a, C, lds, pre);
}

// Arguments the step needs at wave start are separate scalars so the CP preloads them into
// SGPRs (-amdgpu-kernarg-preload-count); the rest (used at the end) is one aggregate.
template <typename Real>
struct HoverTail {
    const HoverConst<Real>* c;
    const HoverReset<Real>* r;
    uint8_t* term;
    uint8_t* trunc;
    float* tobs;
    int32_t* contact_count;
    uint64_t seed;
    int64_t env_offset;
    int B, D, autoreset;
};

// DEF: compiled-in cf2x_consts (the reference default) instead of the device block.
// STG: LDS-staged coalesced obs rows (host: only when E % kStepBlock == 0).
// Launch with kStepBlock threads per workgroup.
// W32: the state fields are addressed by 32-bit byte offsets (host: only while field_offsets_fit(E)).
template <typename Real, int PH, int A, int B, bool DEF, bool STG = false, int CTL = 0, bool HELP = false, bool W32 = true>
__global__ void __launch_bounds__(256) hover_step_kernel(Real* f, float* ring, int32_t* ist, const float* act,
                                                         float* obs, float* rew, int E, HoverTail<Real> t) {
    HoverArgs<Real> a;
    a.c = t.c; a.r = t.r;
    a.f = f; a.ring = ring; a.ist = ist; a.act = act; a.obs = obs; a.rew = rew;
    a.term = t.term; a.trunc = t.trunc; a.tobs = t.tobs; a.mask = nullptr; a.contact_count = t.contact_count;
    a.seed = t.seed; a.env_offset = t.env_offset;
    a.E = E; a.B = t.B; a.D = t.D; a.autoreset = t.autoreset;
    if constexpr (DEF) {
        constexpr HoverConst<Real> C = cf2x_consts<Real>(PH);
        hover_step_body<Real, PH, A, B, C.S, STG, CTL, HELP, 0, W32 ? 1 : 0>(a, C);
    } else {
        hover_step_body<Real, PH, A, B, 0, STG, CTL, HELP, 0, W32 ? 1 : 0>(a, *a.c);
    }
}

// reset kernel (BaseAviary.reset -> _housekeeping -> _computeObs); ring is NOT cleared (Q21)
template <typename Real, int A>
__global__ void __launch_bounds__(256) hover_reset_kernel(HoverArgs<Real> a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E || (a.mask && !a.mask[e])) return;
    const HoverConst<Real>& C = *a.c;
    const int E = a.E;
    const bool dyn = C.physics == ADRP_PHYS_DYN;
    const bool drag = C.physics == ADRP_PHYS_PYB_DRAG || C.physics == ADRP_PHYS_PYB_GND_DRAG_DW;
    Body<Real> b;
    int32_t sc = a.ist[HI_STEP * E + e], ep = a.ist[HI_EPISODE * E + e];
    const int head = a.ist[HI_RING_HEAD * E + e];
    hover_reset_state(a, C, e, b, sc, ep);
    store_body(a, e, b, C.link_lag && !dyn, drag, dyn);
    a.ist[HI_STEP * E + e] = sc;
    a.ist[HI_EPISODE * E + e] = ep;
    float o12[12];
    hover_obs12(C, b, o12);
    const float none[A] = {};
    write_row_generic<A>(a.obs + size_t(e) * a.D, o12, a.ring, a.B, E, e, head, none, false);
}

}  // namespace adrp
