// camera_core.h — the drone camera of the race scene by ray casting (include/adrp.h: adrp_race_camera).
//
// BaseAviary._getDroneImages (BaseAviary.py:569-621) restated for a scene of analytic shapes: the ground
// plane, the gates' and obstacles' URDF boxes and z-axis cylinders (portal.urdf, low_portal.urdf,
// obstacle.urdf: every collision shape is also the link's visual; portal.urdf's visual-only base sphere of
// radius 0.01 is not drawn) and the other drones' collision cylinders.  This header
// holds the one copy of the camera's part table, the view construction and the ray / box / cylinder /
// plane tests; it compiles for the device (camera_kernel.h) and, unchanged, for the host
// (camera_host.cpp, the CPU twin that tests/test_camera.py compares with the numpy reference).
//
// Arithmetic: the view basis and "primitive centre - eye" are formed in the state's precision Real and
// then rounded to float (the difference of the two positions first, then the constant offsets: a
// coordinate of 3 m does not cost the bits of a part 0.3 m away); everything per pixel is float.
// The ray of pixel (x, y) is d = f + x s + y u from the eye, so the ray parameter t of a hit is its
// eye-space depth.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CAM_HD __host__ __device__ inline
#else
#define CAM_HD inline
#endif

namespace adrp_cam {

constexpr double kArm = 0.0397;          // cf2x arm L: eye = pos + (0, 0, L), near = L
constexpr double kNear = kArm, kFar = 1000.0;
constexpr float kTanHalfFov = 0.57735026918962576f;   // tan(30 deg): 60 deg vertical FOV, aspect 1
constexpr float kCosHalfFov = 0.86602540378443865f;
constexpr double kDroneR = 0.06, kDroneHH = 0.0125;   // cf2x_IROS.urdf collision cylinder
constexpr int kGateParts = 5, kObstParts = 2, kMaxGates = 4, kMaxObst = 4, kMaxDrones = 8;
constexpr int kMaxPrims = kMaxGates * kGateParts + kMaxObst * kObstParts + kMaxDrones - 1;   // 35
constexpr int kBox = 0, kCyl = 1;
constexpr int32_t kSegNone = -1;
constexpr float kDepNone = 1.0f;

constexpr uint32_t rgba_(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16) | (255u << 24); }
// floor(255 c + .5) of the URDF material colours
constexpr uint32_t kGrey = rgba_(128, 128, 128), kBlue = rgba_(0, 0, 230), kGreen = rgba_(0, 230, 0),
                   kRed = rgba_(230, 0, 0), kKindaBlue = rgba_(26, 128, 179), kBrown = rgba_(235, 222, 201),
                   kDroneCol = rgba_(128, 128, 128), kGround = rgba_(255, 255, 255), kNothing = 0u;

// one placed primitive, as the pixels read it (20 words)
struct alignas(16) Prim {
    float a[3];      // the eye in the part's frame: -(W (centre - eye))
    float r;         // cylinder radius
    float W[9];      // world -> part rotation, row major
    float h[3];      // half extents (cylinder: h[2] the half height)
    int32_t kind;    // kBox / kCyl
    int32_t seg;     // id + ((link + 1) << 24)
    uint32_t rgba;
    uint32_t pad;
};

struct Cam {
    float f[3], s[3], u[3];
    float eye_z;     // height of the eye over the ground plane
};

struct Pixel {
    float dep;
    int32_t seg;
    uint32_t rgba;
};

// the state planes of adrp_get_state that the camera reads: plane k of a field at p + k * EN, column slot
template <typename Real>
struct Scene {
    int N, G, O;
    int gate_low[kMaxGates];
    size_t EN;
    const Real *pos, *quat, *gates, *obst;
};

// ---- the part table (own frame of the body) -------------------------------------------------------
struct PartDef {
    double off[3], h[3], r;
    int ry;          // rotated by rpy = (0, 1.57, 0) against the body
    int kind, link;
    uint32_t rgba;
};
// part k of a gate: bottom bar (grey), top bar (blue), +x bar (green), -x bar (red), support
CAM_HD PartDef gate_part_def(int k, int low) {
    PartDef p = {{0, 0, 0}, {0.25, 0.025, 0.025}, 0.0, 0, kBox, k, kGrey};
    if (k == 0) p.off[2] = -0.225;
    else if (k == 1) { p.off[2] = 0.225; p.rgba = kBlue; }
    else if (k == 2) { p.off[0] = 0.225; p.ry = 1; p.rgba = kGreen; }
    else if (k == 3) { p.off[0] = -0.225; p.ry = 1; p.rgba = kRed; }
    else if (low) { p.off[2] = -0.4; p.h[0] = 0.075; p.h[1] = 0.075; p.h[2] = 0.125; p.rgba = kBrown; }
    else { p.off[2] = -0.6; p.h[0] = 0; p.h[1] = 0; p.h[2] = 0.4; p.r = 0.05; p.kind = kCyl; p.rgba = kKindaBlue; }
    return p;
}
// part k of an obstacle: the cylinder (the base link, -1), the box (link 0)
CAM_HD PartDef obst_part_def(int k) {
    PartDef p = {{0, 0, 0}, {0, 0, 0.4}, 0.05, 0, kCyl, -1, kKindaBlue};
    if (k == 1) { p.off[2] = -0.4; p.h[0] = 0.075; p.h[1] = 0.075; p.h[2] = 0.125; p.r = 0; p.kind = kBox; p.link = 0; p.rgba = kBrown; }
    return p;
}

CAM_HD int prim_count(int N, int G, int O) { return G * kGateParts + O * kObstParts + N - 1; }

// ---- small algebra --------------------------------------------------------------------------------
template <typename Real>
CAM_HD Real sqrt_(Real x);
template <>
CAM_HD float sqrt_<float>(float x) { return sqrtf(x); }
template <>
CAM_HD double sqrt_<double>(double x) { return sqrt(x); }
template <typename Real>
CAM_HD void sincos_(Real x, Real* s, Real* c);
template <>
CAM_HD void sincos_<float>(float x, float* s, float* c) { *s = sinf(x); *c = cosf(x); }
template <>
CAM_HD void sincos_<double>(double x, double* s, double* c) { *s = sin(x); *c = cos(x); }

// body -> world rotation of a quaternion (x, y, z, w), row major; any non-zero length
template <typename Real>
CAM_HD void quat_rot(const Real q[4], Real R[9]) {
    const Real x = q[0], y = q[1], z = q[2], w = q[3];
    const Real k = Real(2) / (x * x + y * y + z * z + w * w);
    R[0] = Real(1) - k * (y * y + z * z); R[1] = k * (x * y - z * w); R[2] = k * (x * z + y * w);
    R[3] = k * (x * y + z * w); R[4] = Real(1) - k * (x * x + z * z); R[5] = k * (y * z - x * w);
    R[6] = k * (x * z - y * w); R[7] = k * (y * z + x * w); R[8] = Real(1) - k * (x * x + y * y);
}

template <typename Real>
CAM_HD void load_pose(const Scene<Real>& sc, size_t slot, Real pos[3], Real q[4]) {
    for (int k = 0; k < 3; ++k) pos[k] = sc.pos[size_t(k) * sc.EN + slot];
    for (int k = 0; k < 4; ++k) q[k] = sc.quat[size_t(k) * sc.EN + slot];
}

// ---- the view: computeViewMatrix(eye, target, up = world z), computeProjectionMatrixFOV(60, 1, L, 1000) ----
template <typename Real>
CAM_HD Cam make_camera(const Real pos[3], const Real q[4]) {
    Real R[9];
    quat_rot(q, R);
    // target - eye = R (1000, 0, 0) + pos - (pos + (0, 0, L))
    Real f[3] = {Real(1000) * R[0], Real(1000) * R[3], Real(1000) * R[6] - Real(kArm)};
    const Real fn = Real(1) / sqrt_(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (int k = 0; k < 3; ++k) f[k] *= fn;
    // s = normalize(f x (0, 0, 1)), u = s x f
    const Real sn = Real(1) / sqrt_(f[0] * f[0] + f[1] * f[1]);
    const Real s[3] = {f[1] * sn, -f[0] * sn, Real(0)};
    const Real u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    Cam c;
    for (int k = 0; k < 3; ++k) { c.f[k] = float(f[k]); c.s[k] = float(s[k]); c.u[k] = float(u[k]); }
    c.eye_z = float(pos[2] + Real(kArm));
    return c;
}

// ---- primitive idx of (env, drone) slot = e N + n: gates, then obstacles, then the env's other drones ----
// -> the primitive, and its centre relative to the eye with its bounding radius (the frustum cull)
template <typename Real>
CAM_HD void make_prim(const Scene<Real>& sc, size_t slot, int n, int idx, const Real pos[3], Prim& out, float crel[3],
                      float* bound) {
    Real c[3], B[9];      // centre - eye; part -> world rotation
    PartDef d;
    int id;
    const int ng = sc.G * kGateParts, no = sc.O * kObstParts;
    if (idx < ng + no) {
        Real org[3], sy = Real(0), cy = Real(1);
        if (idx < ng) {
            const int g = idx / kGateParts;
            d = gate_part_def(idx - g * kGateParts, sc.gate_low[g]);
            for (int k = 0; k < 3; ++k) org[k] = sc.gates[size_t(4 * g + k) * sc.EN + slot];
            sincos_(sc.gates[size_t(4 * g + 3) * sc.EN + slot], &sy, &cy);
            id = 1 + sc.N + g;
        } else {
            const int o = (idx - ng) / kObstParts;
            d = obst_part_def(idx - ng - o * kObstParts);
            for (int k = 0; k < 3; ++k) org[k] = sc.obst[size_t(3 * o + k) * sc.EN + slot];
            id = 1 + sc.N + sc.G + o;
        }
        // B = Rz(yaw) [Ry(1.57)]
        const Real c157 = Real(0.0007963267107332633), s157 = Real(0.9999996829318346);
        if (d.ry) {
            B[0] = cy * c157; B[1] = -sy; B[2] = cy * s157;
            B[3] = sy * c157; B[4] = cy; B[5] = sy * s157;
            B[6] = -s157; B[7] = Real(0); B[8] = c157;
        } else {
            B[0] = cy; B[1] = -sy; B[2] = Real(0);
            B[3] = sy; B[4] = cy; B[5] = Real(0);
            B[6] = Real(0); B[7] = Real(0); B[8] = Real(1);
        }
        const Real ox = Real(d.off[0]), oy = Real(d.off[1]), oz = Real(d.off[2]);
        c[0] = (org[0] - pos[0]) + (cy * ox - sy * oy);
        c[1] = (org[1] - pos[1]) + (sy * ox + cy * oy);
        c[2] = (org[2] - pos[2]) + (oz - Real(kArm));
    } else {
        const int j = idx - ng - no, m = j < n ? j : j + 1;      // the env's other drones in order
        Real p[3], q[4];
        load_pose(sc, slot - size_t(n) + size_t(m), p, q);
        quat_rot(q, B);
        for (int k = 0; k < 3; ++k) c[k] = p[k] - pos[k];
        c[2] -= Real(kArm);
        d = PartDef{{0, 0, 0}, {0, 0, kDroneHH}, kDroneR, 0, kCyl, -1, kDroneCol};
        id = 1 + m;
    }
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) out.W[3 * i + k] = float(B[3 * k + i]);      // W = B^T
        out.a[i] = float(-(B[i] * c[0] + B[3 + i] * c[1] + B[6 + i] * c[2]));
        out.h[i] = float(d.h[i]);
        crel[i] = float(c[i]);
    }
    out.r = float(d.r);
    out.kind = d.kind;
    out.seg = id + ((d.link + 1) << 24);
    out.rgba = d.rgba;
    out.pad = 0;
    *bound = d.kind == kCyl ? sqrtf(out.r * out.r + out.h[2] * out.h[2])
                            : sqrtf(out.h[0] * out.h[0] + out.h[1] * out.h[1] + out.h[2] * out.h[2]);
}

// can a ball (centre relative to the eye, radius) reach into the view pyramid past the near plane?
// (a conservative test: every pixel's ray lies inside the pyramid)
CAM_HD bool ball_in_view(const Cam& c, const float crel[3], float radius) {
    const float rb = radius * 1.001f + 1e-4f;
    const float z = crel[0] * c.f[0] + crel[1] * c.f[1] + crel[2] * c.f[2];
    const float x = crel[0] * c.s[0] + crel[1] * c.s[1] + crel[2] * c.s[2];
    const float y = crel[0] * c.u[0] + crel[1] * c.u[1] + crel[2] * c.u[2];
    if (z + rb < float(kNear)) return false;
    if ((fabsf(x) - z * kTanHalfFov) * kCosHalfFov > rb) return false;
    if ((fabsf(y) - z * kTanHalfFov) * kCosHalfFov > rb) return false;
    return true;
}

// ---- ray tests: entry parameter of the ray a + t dl into the primitive, or a negative number ----
CAM_HD bool slab_(float a, float d, float h, float& lo, float& hi) {
    if (d == 0.0f) return fabsf(a) <= h;
    const float inv = 1.0f / d;
    float t1 = (-h - a) * inv, t2 = (h - a) * inv;
    if (t1 > t2) { const float t = t1; t1 = t2; t2 = t; }
    if (t1 > lo) lo = t1;
    if (t2 < hi) hi = t2;
    return true;
}

CAM_HD float ray_prim(const Prim& p, const float d[3]) {
    const float dl[3] = {p.W[0] * d[0] + p.W[1] * d[1] + p.W[2] * d[2], p.W[3] * d[0] + p.W[4] * d[1] + p.W[5] * d[2],
                         p.W[6] * d[0] + p.W[7] * d[1] + p.W[8] * d[2]};
    float lo = -INFINITY, hi = INFINITY;
    if (!slab_(p.a[2], dl[2], p.h[2], lo, hi)) return -1.0f;
    if (p.kind == kBox) {
        if (!slab_(p.a[0], dl[0], p.h[0], lo, hi)) return -1.0f;
        if (!slab_(p.a[1], dl[1], p.h[1], lo, hi)) return -1.0f;
    } else {
        // |a + t dl|^2 = r^2 in the xy plane; the discriminant as r^2 |dl|^2 - (a x dl)^2 (no
        // cancellation of two numbers of the size of the distance squared)
        const float qa = dl[0] * dl[0] + dl[1] * dl[1], qb = p.a[0] * dl[0] + p.a[1] * dl[1];
        if (qa == 0.0f) {
            if (p.a[0] * p.a[0] + p.a[1] * p.a[1] > p.r * p.r) return -1.0f;
        } else {
            const float cr = p.a[0] * dl[1] - p.a[1] * dl[0];
            const float disc = p.r * p.r * qa - cr * cr;
            if (disc < 0.0f) return -1.0f;
            const float sq = sqrtf(disc), inv = 1.0f / qa;
            const float t3 = (-qb - sq) * inv, t4 = (-qb + sq) * inv;
            if (t3 > lo) lo = t3;
            if (t4 < hi) hi = t4;
        }
    }
    return lo <= hi ? lo : -1.0f;
}

// depth-buffer value of eye-space depth z: far / (far - near) (1 - near / z)
CAM_HD float depth_buffer(float z) {
    return float(kFar / (kFar - kNear)) * (1.0f - float(kNear) / z);
}

// NDC of pixel centre k of n
CAM_HD float pixel_ndc(int k, int n) { return 2.0f * (float(k) + 0.5f) / float(n) - 1.0f; }

// pixel (row i from the top, column j): the nearest entry with near <= t <= far wins; a primitive
// entered before the near plane is not seen
CAM_HD Pixel shade(const Cam& c, int i, int j, int width, int height, const Prim* tab, int count) {
    const float x = pixel_ndc(j, width) * kTanHalfFov, y = -pixel_ndc(i, height) * kTanHalfFov;
    const float d[3] = {c.f[0] + x * c.s[0] + y * c.u[0], c.f[1] + x * c.s[1] + y * c.u[1], c.f[2] + x * c.s[2] + y * c.u[2]};
    float best = float(kFar);
    Pixel px = {kDepNone, kSegNone, kNothing};
    bool hit = false;
    if (d[2] < 0.0f) {
        const float t = c.eye_z / -d[2];
        if (t >= float(kNear) && t <= best) { best = t; hit = true; px.seg = 0; px.rgba = kGround; }
    }
    for (int k = 0; k < count; ++k) {
        const float t = ray_prim(tab[k], d);
        if (t >= float(kNear) && t < best) { best = t; hit = true; px.seg = tab[k].seg; px.rgba = tab[k].rgba; }
    }
    if (hit) px.dep = depth_buffer(best);
    return px;
}

}  // namespace adrp_cam
