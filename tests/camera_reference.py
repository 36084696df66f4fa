"""numpy reference of the drone camera (include/adrp.h adrp_race_camera) and the constructed
scenes that tests/test_camera.py (CPU twin) and tests/test_camera_gpu.py (kernel) compare against it.

The camera model is BaseAviary._getDroneImages restated (pybullet's documented computeViewMatrix /
computeProjectionMatrixFOV / depth-buffer conventions):
  eye = pos + (0, 0, L), L = 0.0397; f = normalize(R (1000, 0, 0) + pos - eye); s = normalize(f x z); u = s x f;
  pixel (row i from the top, column j): x = (2 (j + .5) / W - 1) tan 30, y = (1 - 2 (i + .5) / H) tan 30,
  ray d = f + x s + y u from the eye, so t is the eye-space depth; the nearest entry with near <= t <= far wins;
  dep = far / (far - near) (1 - near / t), 1 where nothing is hit.
The shapes come from tests/race_scenes.py (placed_parts: the URDF parts as the race oracle places them; the
drones' collision cylinders), the segmentation values and colours from the URDF link order and materials.

Everything is evaluated in float64, and again in float32 (primitive centre - eye and the view basis formed in
float64, then rounded; every per-pixel operation in float32): the largest float32-to-float64 difference on
decided pixels, over every ray the tests cast from the poses, sets the depth bars of the tests (bars()).

A pixel is *decided* unless
  (a) the ray of the same pixel shifted by +-1e-3 in x or in y (NDC units) hits another primitive,
  (b) the runner-up primitive's t is within 1e-3 t of the winner's (the bars of a gate overlap at the
      corners and share a face plane: the link there is a tie), or
  (c) the hit is the ground beyond 50 m (the horizon row).
Undecided pixels are left out of the comparisons; at most CAP of an image's pixels may be undecided.
"""
import numpy as np

import race_scenes as RS
from gym_pybullet_adrp_amd.camera import FAR, NEAR, linear_depth
from gym_pybullet_adrp_amd.envs import tracks

L = 0.0397
TAN30 = np.tan(np.pi / 6)
SHIFT, TIE, HORIZON, CAP = 1e-3, 1e-3, 50.0, 0.08
N = 2
SEED = 2024                                    # of the constructed set
SIZES = ((64, 48), (17, 9), (1, 1))            # (W, H)

GREY, BLUE, GREEN, RED = (128, 128, 128, 255), (0, 0, 230, 255), (0, 230, 0, 255), (230, 0, 0, 255)
KINDABLUE, BROWN, WHITE, NONE = (26, 128, 179, 255), (235, 222, 201, 255), (255, 255, 255, 255), (0, 0, 0, 0)
GATE_COLOURS = {0: [GREY, BLUE, GREEN, RED, KINDABLUE], 1: [GREY, BLUE, GREEN, RED, BROWN]}
OBST_COLOURS, OBST_LINKS = [KINDABLUE, BROWN], [-1, 0]
GATE_LOW = [int(g[6] > 0) for g in tracks._BASE["gates"]]


def seg_value(body, link):
    return body + ((link + 1) << 24)


def quat_from_rpy(r, p, y):
    sr, cr, sp, cp, sy, cy = np.sin(r / 2), np.cos(r / 2), np.sin(p / 2), np.cos(p / 2), np.sin(y / 2), np.cos(y / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


class Env:
    """one env of the constructed set: N drone poses, the four gates (x, y, z, yaw), the four obstacles (x, y, z);
    every value is float32-representable, so float32 and float64 state planes hold the same numbers"""

    def __init__(self, pos, quat, gates, obst):
        self.pos, self.quat = RS.f32(pos), RS.f32(quat)
        self.gates, self.obst = RS.f32(gates), RS.f32(obst)


def primitives(env, n):
    """the scene of drone n's camera: [(label, cyl, centre, part -> world rotation, half extents, radius, seg, rgba)]"""
    out = []
    for g in range(4):
        low = GATE_LOW[g]
        for k, s in enumerate(RS.placed_parts(0, low, env.gates[g])):
            out.append((("gate", k, low), int(s[0]), np.array(s[1:4]), np.array(s[4:13]).reshape(3, 3), np.array(s[13:16]),
                        s[16], seg_value(1 + N + g, k), GATE_COLOURS[low][k]))
    for o in range(4):
        for k, s in enumerate(RS.placed_parts(1, 0, [*env.obst[o], 0.0])):
            out.append((("obstacle", OBST_LINKS[k], 0), int(s[0]), np.array(s[1:4]), np.array(s[4:13]).reshape(3, 3),
                        np.array(s[13:16]), s[16], seg_value(1 + N + 4 + o, OBST_LINKS[k]), OBST_COLOURS[k]))
    for m in range(N):
        if m != n:
            s = RS.cyl_shape(env.pos[m], RS.rot_from_quat(env.quat[m]))
            out.append((("drone", -1, 0), 1, np.array(s[1:4]), np.array(s[4:13]).reshape(3, 3), np.array(s[13:16]), s[16],
                        seg_value(1 + m, -1), GREY))
    return out


def view(pos, quat):
    """eye, f, s, u (float64)"""
    R = RS.rot_from_quat(quat)
    eye = np.asarray(pos, float) + [0, 0, L]
    f = R @ [1000.0, 0, 0] + pos - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, [0, 0, 1.0])
    s /= np.linalg.norm(s)
    return eye, f, s, np.cross(s, f)


def _slab(T, a, dk, h, lo, hi, miss):
    zero = dk == 0
    inv = T(1) / np.where(zero, T(1), dk)
    t1, t2 = (-h - a) * inv, (h - a) * inv
    lo = np.maximum(lo, np.where(zero, T(-np.inf), np.minimum(t1, t2)))
    hi = np.minimum(hi, np.where(zero, T(np.inf), np.maximum(t1, t2)))
    return lo, hi, miss | (zero & (abs(a) > h))


def ray_prim(T, a, Wm, h, r, cyl, d):
    """entry parameter [P] of the rays a + t (Wm d) into the box / z cylinder, inf where they miss"""
    dl = d @ Wm.T
    lo, hi = np.full(len(d), -np.inf, T), np.full(len(d), np.inf, T)
    miss = np.zeros(len(d), bool)
    lo, hi, miss = _slab(T, a[2], dl[:, 2], h[2], lo, hi, miss)
    if not cyl:
        for k in (0, 1):
            lo, hi, miss = _slab(T, a[k], dl[:, k], h[k], lo, hi, miss)
    else:
        qa, qb = dl[:, 0] ** 2 + dl[:, 1] ** 2, a[0] * dl[:, 0] + a[1] * dl[:, 1]
        cr = a[0] * dl[:, 1] - a[1] * dl[:, 0]
        disc = r * r * qa - cr * cr
        zero = qa == 0
        miss |= (zero & (a[0] * a[0] + a[1] * a[1] > r * r)) | (~zero & (disc < 0))
        sq, inv = np.sqrt(np.maximum(disc, T(0))), T(1) / np.where(zero, T(1), qa)
        lo = np.maximum(lo, np.where(zero, T(-np.inf), (-qb - sq) * inv))
        hi = np.minimum(hi, np.where(zero, T(np.inf), (-qb + sq) * inv))
    return np.where(miss | (lo > hi), T(np.inf), lo)


def cast(env, n, W, H, T=np.float64, dx=0.0, dy=0.0):
    """t [1 + K, H*W] of the ground and the K primitives (inf: not seen), every pixel shifted by (dx, dy) NDC"""
    eye, f, s, u = view(env.pos[n], env.quat[n])
    prims = primitives(env, n)
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    x = ((T(2) * (j.ravel().astype(T) + T(0.5)) / T(W) - T(1)) + T(dx)) * T(TAN30)
    y = -((T(2) * (i.ravel().astype(T) + T(0.5)) / T(H) - T(1)) + T(dy)) * T(TAN30)
    f, s, u = f.astype(T), s.astype(T), u.astype(T)
    d = f[None, :] + x[:, None] * s[None, :] + y[:, None] * u[None, :]
    near, far = T(NEAR), T(FAR)
    ts = np.full((1 + len(prims), H * W), np.inf, T)
    down = d[:, 2] < 0
    tg = T(eye[2]) / np.where(down, -d[:, 2], T(1))
    ts[0] = np.where(down & (tg >= near) & (tg <= far), tg, T(np.inf))
    for k, (_, cyl, c, B, h, r, _, _) in enumerate(prims):
        a = (-(B.T @ (c - eye))).astype(T)
        t = ray_prim(T, a, B.T.astype(T), h.astype(T), T(r), cyl, d)
        ts[1 + k] = np.where((t >= near) & (t < far), t, T(np.inf))
    return ts, prims


def depth_buffer(t, T=np.float64):
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(t), T(FAR / (FAR - NEAR)) * (T(1) - T(NEAR) / t), T(1)).astype(T)


def reference(env, n, W, H):
    """dict of [H, W] arrays: seg, rgb [H, W, 4], dep / z (float64), dep32 / z32 (the float32 evaluation),
    decided, label (index into LABELS of the winner), plus `objects` (winner is a gate, obstacle or drone)"""
    ts, prims = cast(env, n, W, H)
    order = np.argsort(ts, axis=0, kind="stable")
    win = order[0]
    px = np.arange(H * W)
    t1, t2 = ts[win, px], ts[order[1], px]
    hit = np.isfinite(t1)
    win = np.where(hit, win, -1)
    with np.errstate(invalid="ignore"):
        undecided = hit & np.isfinite(t2) & (t2 - t1 <= TIE * t1)                    # (b)
    undecided |= (win == 0) & (t1 > HORIZON)                                         # (c)
    for dx, dy in ((SHIFT, 0), (-SHIFT, 0), (0, SHIFT), (0, -SHIFT)):                # (a)
        tk, _ = cast(env, n, W, H, dx=dx, dy=dy)
        wk = np.where(np.isfinite(tk.min(0)), tk.argmin(0), -1)
        undecided |= wk != win
    segs = np.array([-1, 0] + [p[6] for p in prims])
    cols = np.array([NONE, WHITE] + [p[7] for p in prims], np.uint8)
    labels = np.array([LABELS.index(("sky", -1, 0)), LABELS.index(("ground", -1, 0))] + [LABELS.index(p[0]) for p in prims])
    dep = depth_buffer(np.where(hit, t1, np.inf))
    # the float32 evaluation: its own winner's depth (on decided pixels the same primitive)
    ts32, _ = cast(env, n, W, H, T=np.float32)
    t32 = ts32.min(0)
    win32 = np.where(np.isfinite(t32), ts32.argmin(0), -1)
    dep32 = depth_buffer(t32, np.float32)
    sh = (H, W)
    return dict(seg=segs[win + 1].astype(np.int32).reshape(sh), rgb=cols[win + 1].reshape(H, W, 4), dep=dep.reshape(sh),
                z=np.where(hit, t1, np.inf).reshape(sh), dep32=dep32.reshape(sh), z32=linear_depth(dep32).reshape(sh),
                same32=(win32 == win).reshape(sh), decided=(~undecided).reshape(sh), label=labels[win + 1].reshape(sh),
                objects=(win >= 1).reshape(sh))


# every (kind, link[, low]) pair of the scene, the ground and the sky
LABELS = [("gate", k, low) for low in (0, 1) for k in range(5)] + [("obstacle", -1, 0), ("obstacle", 0, 0), ("drone", -1, 0),
                                                                  ("ground", -1, 0), ("sky", -1, 0)]


# ---- the constructed set -------------------------------------------------------------------------------------
def _look(pos, at, rng, tilt=0.4):
    """quaternion of a drone at pos whose camera looks at `at`, tilted by up to +-tilt in roll and pitch"""
    d = np.asarray(at, float) - (np.asarray(pos, float) + [0, 0, L])
    yaw, pitch = np.arctan2(d[1], d[0]), -np.arctan2(d[2], np.hypot(d[0], d[1]))
    return quat_from_rpy(rng.uniform(-tilt, tilt), pitch + rng.uniform(-tilt, tilt), yaw)


def constructed_envs():
    """12 envs x 2 drones = 24 images on the level0 track (per env shifted like level2's gate / obstacle offsets):
    three poses 0.4 to 1.5 m in front of each gate and two per obstacle, tilted by up to +-0.4 rad in roll and
    pitch; a second drone 0.5 m ahead, looking back; one pose pitched down 1.2 rad; one looking away from everything"""
    if _SET:
        return _SET
    G0 = np.array([[g[0], g[1], g[2], g[5]] for g in tracks._BASE["gates"]])
    O0 = np.array([o[:3] for o in tracks._BASE["obstacles"]])
    views = []          # (what, index, distance, side, aim height offset)
    for g in range(4):
        for k, (dist, dz) in enumerate(((0.45, 0.0), (0.9, -0.15), (1.45, -0.35))):
            views.append(("gate", g, dist, (1, -1)[(g + k) % 2], dz))
    for o in range(4):
        for dist, dz in ((0.5, 0.1), (1.2, -0.3)):
            views.append(("obstacle", o, dist, 1, dz))
    views += [("ahead", 1, 1.0, 1, -0.1), ("behind", 0, 0, 0, 0), ("down", 0, 0, 0, 0), ("away", 0, 0, 0, 0)]
    for e in range(len(views) // 2):
        # an env is drawn again (its own stream, so nothing else changes) until the reference finds every image
        # of it within the cap at every size; the code under test has no part in this
        for attempt in range(50):
            env = _draw_env(np.random.default_rng([SEED, e, attempt]), views[2 * e:2 * e + N], G0, O0)
            refs = {(W, H): [reference(env, n, W, H) for n in range(N)] for W, H in SIZES}
            if all(1 - r["decided"].mean() <= CAP for rs in refs.values() for r in rs):
                break
        else:
            raise AssertionError(f"constructed env {e}: no draw within the cap of undecided pixels")
        _SET.append(env)
        for size, rs in refs.items():
            _REF.setdefault(size, []).append(rs)
    return _SET


def _draw_env(rng, views, G0, O0):
    gates, obst = G0.copy(), O0.copy()
    gates[:, :3] += rng.uniform(-0.15, 0.15, (4, 3))
    obst += rng.uniform(-0.15, 0.15, (4, 3))
    pos, quat = np.zeros((N, 3)), np.zeros((N, 4))
    for n in range(N):
        what, k, dist, side, dz = views[n]
        if what in ("gate", "ahead"):
            c, yaw = gates[k, :3], gates[k, 3]
            pos[n] = c + side * dist * np.array([-np.sin(yaw), np.cos(yaw), 0]) + [0, 0, rng.uniform(-0.1, 0.1)]
            quat[n] = _look(pos[n], c + [0, 0, dz], rng, 0.4 if what == "gate" else 0.1)
        elif what == "obstacle":
            th = rng.uniform(-np.pi, np.pi)
            pos[n] = obst[k] + dist * np.array([np.cos(th), np.sin(th), 0]) + [0, 0, rng.uniform(-0.1, 0.2)]
            quat[n] = _look(pos[n], obst[k] + [0, 0, dz], rng)
        elif what == "behind":      # 0.5 m ahead of drone 0 along its view, looking back at it
            _, f, _, _ = view(pos[0], quat[0])
            pos[n] = pos[0] + 0.5 * f + [0, 0, 0.03]
            quat[n] = _look(pos[n], pos[0], rng, 0.1)
        elif what == "down":
            pos[n] = [0.2, -0.3, 1.2]
            quat[n] = quat_from_rpy(0.1, 1.2, 0.7 + rng.uniform(-0.2, 0.2))
        else:
            pos[n] = [2.5, 2.5, 1.0]
            quat[n] = quat_from_rpy(0.05, -0.2, np.pi / 4 + rng.uniform(-0.2, 0.2))
    return Env(pos, quat, gates, obst)


_SET, _REF, _BARS = [], {}, []


def references(W, H):
    """[env][drone] reference() of the constructed set at W x H, computed once per process"""
    envs = constructed_envs()
    if (W, H) not in _REF:
        _REF[(W, H)] = [[reference(env, n, W, H) for n in range(N)] for env in envs]
    return _REF[(W, H)]


def planes(envs, dtype):
    """(pos [3, E*N], quat [4, E*N], gates [16, E*N], obstacles [12, E*N]) as adrp_get_state lays them out"""
    pos = np.concatenate([e.pos for e in envs]).T
    quat = np.concatenate([e.quat for e in envs]).T
    gates = np.repeat(np.stack([e.gates.ravel() for e in envs]), N, axis=0).T
    obst = np.repeat(np.stack([e.obst.ravel() for e in envs]), N, axis=0).T
    return tuple(np.ascontiguousarray(a, dtype) for a in (pos, quat, gates, obst))


def check_set(W, H, coverage=True):
    """the conditions on the set, judged by the reference alone: every image within CAP undecided; at 64 x 48 at
    least 10 % of all pixels on a gate, an obstacle or a drone and every label the decided answer of >= 20 pixels"""
    refs = [r for env in references(W, H) for r in env]
    for k, r in enumerate(refs):
        share = 1 - r["decided"].mean()
        assert share <= CAP, f"image {k} at {W}x{H}: {share:.3f} of the pixels undecided"
    if coverage:
        objects = np.mean([r["objects"].mean() for r in refs])
        assert objects >= 0.10, f"only {objects:.3f} of the pixels hit a gate, an obstacle or a drone"
        count = np.zeros(len(LABELS), int)
        for r in refs:
            count += np.bincount(r["label"][r["decided"]], minlength=len(LABELS))
        assert count.min() >= 20, f"labels with fewer than 20 decided pixels: {[LABELS[k] for k in np.flatnonzero(count < 20)]}"
    return refs


def bars():
    """(dep bar, relative linear-depth bar, measured dep difference, measured linear-depth difference): 4 x the
    largest float32-to-float64 difference of the reference on decided pixels, floors 2^-22.

    The largest difference is a property of the poses, so it is taken over every ray the tests cast from them
    (all of SIZES together), not per image size: the 24 rays of the 1 x 1 images alone estimate a maximum from 24
    samples (6.7e-6 relative on linear depth, where 64 x 48 finds 5.1e-5 on the same poses), which lies below what
    the float32 dep format itself resolves: one ulp of dep near 1 is 6e-8, and linear_depth turns a dep error e
    into a relative depth error e z / near, 4e-5 for the ground 28 m away."""
    if not _BARS:
        ddep, dz = 0.0, 0.0
        for W, H in SIZES:
            for r in (r for env in references(W, H) for r in env):
                m = r["decided"]
                assert r["same32"][m].all(), "the float32 reference chose another primitive on a decided pixel"
                ddep = max(ddep, float(np.abs(r["dep32"][m].astype(np.float64) - r["dep"][m]).max(initial=0)))
                h = m & np.isfinite(r["z"])
                dz = max(dz, float((np.abs(r["z32"][h].astype(np.float64) - r["z"][h]) / r["z"][h]).max(initial=0)))
        _BARS.extend([max(4 * ddep, 2.0 ** -22), max(4 * dz, 2.0 ** -22), ddep, dz])
    return tuple(_BARS)


def compare(refs, dep, seg, rgb, dep_bar, z_bar, what=""):
    """images [len(refs), H, W(, 4)] against the references on decided pixels: seg and rgb exact, dep within
    dep_bar, linear_depth(dep) within z_bar relative; returns the measured (dep, z) differences"""
    worst = [0.0, 0.0]
    for k, r in enumerate(refs):
        m = r["decided"]
        assert (seg[k][m] == r["seg"][m]).all(), f"{what} image {k}: seg differs on {(seg[k][m] != r['seg'][m]).sum()} decided pixels"
        assert (rgb[k][m] == r["rgb"][m]).all(), f"{what} image {k}: rgb differs on decided pixels"
        worst[0] = max(worst[0], float(np.abs(dep[k][m].astype(np.float64) - r["dep"][m]).max(initial=0)))
        h = m & np.isfinite(r["z"])
        z = linear_depth(dep[k][h]).astype(np.float64)
        worst[1] = max(worst[1], float((np.abs(z - r["z"][h]) / r["z"][h]).max(initial=0)))
    print(f"{what}: dep diff {worst[0]:.3g} (bar {dep_bar:.3g}), linear depth diff {worst[1]:.3g} relative (bar {z_bar:.3g})")
    assert worst[0] <= dep_bar and worst[1] <= z_bar, (what, worst, dep_bar, z_bar)
    return worst


# ---- the CPU twin (csrc/camera_host) ---------------------------------------------------------------------------
def build_camera_host():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "gym_pybullet_adrp_amd", "csrc"), "camera_host"])
    return os.path.join(root, "gym_pybullet_adrp_amd", "camera_host")


def run_camera_host(envs, W, H, tmpdir, dtype=np.float64, cull=1):
    """csrc/camera_host on the envs: (dep [E*N, H, W] float32, seg int32, rgb [E*N, H, W, 4] uint8)"""
    import os
    import subprocess
    exe = build_camera_host()
    hd = np.zeros(16, np.int32)
    hd[:6] = len(envs), N, W, H, 4, 4
    hd[6:10] = GATE_LOW
    hd[10], hd[11] = int(dtype == np.float64), cull
    fin, fout = os.path.join(str(tmpdir), "camera_scene.bin"), os.path.join(str(tmpdir), "camera_out.bin")
    with open(fin, "wb") as f:
        f.write(hd.tobytes())
        for a in planes(envs, dtype):
            f.write(a.tobytes())
    subprocess.check_call([exe, fin, fout])
    px = len(envs) * N * H * W
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == 12 * px
    dep = raw[:4 * px].view(np.float32).reshape(-1, H, W)
    seg = raw[4 * px:8 * px].view(np.int32).reshape(-1, H, W)
    rgb = raw[8 * px:].reshape(-1, H, W, 4)
    return dep, seg, rgb
