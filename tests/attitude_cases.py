"""Constructed attitudes for the Euler-angle edges of the step kernels: the gimbal-lock branches
(|sin pitch| >= 0.99999), the roll / yaw seam at +-pi, quaternions with w < 0, and the longdouble
references they are held against.  No GPU; shared by test_attitude_edges.py, test_math_gpu.py and
test_attitude_edges_gpu.py.

Quaternions are xyzw.  Each case comes from a numpy.longdouble getQuaternionFromEuler (or is an
explicit quaternion), is rounded to the env's real type by `table(dtype)`, and appears as q and -q.
sarg = -2 (x z - w y) = sin pitch decides the branch of getEulerFromQuaternion:

  generic side   |sarg| <= 0.99998
  gimbal side    |sarg| >= 0.9999955

so no case sits within 4e-6 of the 0.99999 threshold and the float kernels, the double kernels and
the oracle all take the same branch of the same (rounded) quaternion.
"""
import numpy as np

L = np.longdouble
PI = 4 * np.arctan(L(1))
THRESH = L("0.99999")
MARGIN = L("4e-6")
GENERIC_MAX = L("0.99998")
GIMBAL_MIN = L("0.9999955")

CLASSES = ("generic", "near", "gimbal")     # near: generic branch, pitch within 1e-2 of +-pi/2


def quat_from_euler_ld(rpy):
    """pybullet getQuaternionFromEuler in longdouble; rpy [..., 3] -> xyzw [..., 4]"""
    rpy = np.asarray(rpy, L)
    hr, hp, hy = rpy[..., 0] / 2, rpy[..., 1] / 2, rpy[..., 2] / 2
    sr, cr, sp, cp, sy, cy = np.sin(hr), np.cos(hr), np.sin(hp), np.cos(hp), np.sin(hy), np.cos(hy)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], -1)


def sarg_of(q, dtype=L):
    q = np.asarray(q, dtype)
    return dtype(-2) * (q[..., 0] * q[..., 2] - q[..., 3] * q[..., 1])


def euler_from_quat(q, dtype=L, atan2=np.arctan2, asin=np.arcsin):
    """pybullet getEulerFromQuaternion with its two gimbal branches, every operation in `dtype`
    (longdouble: the reference; float64 / float32: the same formula's own rounding error)"""
    q = np.asarray(q, dtype)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two = dtype(2)
    sarg = dtype(-2) * (x * z - w * y)
    sqx, sqy, sqz, squ = x * x, y * y, z * z, w * w
    with np.errstate(invalid="ignore"):
        roll = atan2(two * (y * z + w * x), squ - sqx - sqy + sqz)
        pitch = asin(np.clip(sarg, dtype(-1), dtype(1)))
        yaw = atan2(two * (x * y + w * z), squ + sqx - sqy - sqz)
    half_pi = dtype(PI / 2)
    lo, hi = sarg <= dtype(-0.99999), sarg >= dtype(0.99999)
    zero = np.zeros_like(roll)
    roll = np.where(lo | hi, zero, roll)
    pitch = np.where(lo, -half_pi, np.where(hi, half_pi, pitch))
    yaw = np.where(lo, two * atan2(x, -y), np.where(hi, two * atan2(-x, y), yaw))
    return np.stack([roll, pitch, yaw], -1).astype(dtype)


def circle_diff(a, b):
    """a - b on the circle, in longdouble, in [-pi, pi]"""
    d = np.asarray(a, L) - np.asarray(b, L)
    return d - 2 * PI * np.round(d / (2 * PI))


def rpy_err(got, ref):
    """|got - ref| per angle: roll and yaw on the circle, pitch plain; [..., 3] longdouble"""
    got, ref = np.asarray(got, L), np.asarray(ref, L)
    d = np.abs(got - ref)
    c = np.abs(circle_diff(got, ref))
    return np.stack([c[..., 0], d[..., 1], c[..., 2]], -1)


def rpy_rel_err(got, ref, floor=1e-3):
    """the step-parity measure of an obs row's rpy block: |got - ref|_2 / max(|ref|_2, floor), the
    difference taken on the circle for roll and yaw"""
    e = np.sqrt((rpy_err(got, ref) ** 2).sum(-1))
    return e / np.maximum(np.sqrt((np.asarray(ref, L) ** 2).sum(-1)), L(floor))


def _cases():
    rng = np.random.default_rng(20240607)
    out = []                                    # (name, side, class, quaternion longdouble)

    def rpy(name, side, cls, r, p, y):
        out.append((name, side, cls, quat_from_euler_ld([L(r), L(p), L(y)])))

    def draw():
        return L(rng.uniform(-3.1, 3.1)), L(rng.uniform(-3.1, 3.1))

    rpy("identity", "generic", "generic", 0, 0, 0)
    for s in (1, -1):
        sg = "+" if s > 0 else "-"
        for nm, a in (("pi", PI), ("pi-1e-6", PI - L("1e-6")), ("pi-1e-3", PI - L("1e-3")), ("3pi/4", 3 * PI / 4),
                      ("pi/2", PI / 2)):
            rpy(f"yaw{sg}{nm}", "generic", "generic", 0, 0, s * a)
        for nm, a in (("pi", PI), ("pi-1e-3", PI - L("1e-3")), ("2.5", L("2.5")), ("pi/2", PI / 2)):
            rpy(f"roll{sg}{nm}", "generic", "generic", s * a, 0, 0)
        for nm, a, cls in (("0.4", L("0.4"), "generic"), ("1.0", L("1.0"), "generic"), ("1.5", L("1.5"), "generic"),
                           ("pi/2-1e-2", PI / 2 - L("1e-2"), "near"), ("pi/2-6.5e-3", PI / 2 - L("6.5e-3"), "near")):
            for k in range(3):
                r, y = draw()
                rpy(f"pitch{sg}{nm}#{k}", "generic", cls, r, s * a, y)
        for nm, d in (("0", L(0)), ("1e-4", L("1e-4")), ("1e-3", L("1e-3")), ("3e-3", L("3e-3"))):
            for k in range(3):
                r, y = draw()
                rpy(f"gimbal{sg}(pi/2-{nm})#{k}", "gimbal", "gimbal", r, s * (PI / 2 - d), y)
        h = np.sqrt(L(0.5))
        out.append((f"gimbal{sg}exact", "gimbal", "gimbal", np.array([0, s * h, 0, h], L)))
    for nm, q in (("q(1,0,0,0)", [1, 0, 0, 0]), ("q(0,1,0,0)", [0, 1, 0, 0]), ("q(0,0,1,0)", [0, 0, 1, 0]),
                  ("q(.5,.5,.5,.5)", [0.5, 0.5, 0.5, 0.5])):
        out.append((nm, "generic", "generic", np.array(q, L)))
    both = []
    for name, side, cls, q in out:
        both.append((name, side, cls, q))
        both.append(("-" + name, side, cls, -q))
    return both


CASES = _cases()
NAMES = [c[0] for c in CASES]
SIDE = np.array([c[1] for c in CASES])
CLASS = np.array([c[2] for c in CASES])
QUAT_LD = np.stack([c[3] for c in CASES])                   # [K, 4] longdouble, unrounded

# the fp32 env tests drop exactly this pair if the float32 evaluation of the reference formula from
# the float32 quaternion leaves half the step-parity bar there (test_attitude_edges.py decides and
# states it); nothing else may be dropped
FP32_DROPPABLE = "pi/2-6.5e-3"


def table(dtype):
    """the cases' quaternions rounded to `dtype` ([K, 4]) and the longdouble reference angles of
    those rounded quaternions ([K, 3])"""
    q = QUAT_LD.astype(dtype)
    return q, euler_from_quat(q.astype(L))


def select(side=None, cls=None):
    m = np.ones(len(CASES), bool)
    if side is not None:
        m &= SIDE == side
    if cls is not None:
        m &= CLASS == cls
    return np.flatnonzero(m)


def random_unit_quats(rng, n, keep_margin=True):
    """n random unit quaternions (longdouble-normalised float64 draws), those within the 4e-6 margin
    of the branch threshold removed"""
    q = rng.normal(size=(n, 4)).astype(L)
    q /= np.sqrt((q * q).sum(-1, keepdims=True))
    if keep_margin:
        for dt in (np.float32, np.float64):
            s = np.abs(sarg_of(q.astype(dt).astype(L)))
            q = q[np.abs(s - THRESH) > MARGIN]
    return q


# ---- numpy float32 emulation of the fp32 fast forms (csrc/adrp_device.h) -------------------------
# every operation rounds to float32 as the kernel's does, with the IEEE division / sqrt in place of
# v_rcp_f32 / v_sqrt_f32 (1 ulp): the floors the GPU bars rest on
F = np.float32
ATAN_COEF = [F(0.0028487828094512224), F(-0.016064105555415154), F(0.04268398508429527), F(-0.07503638416528702),
             F(0.10640615969896317), F(-0.1420356035232544), F(0.19992607831954956), F(-0.3333307206630707), F(1.0)]


def fatan2_f32(y, x, rcp_ulps=0):
    y, x = np.asarray(y, F), np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rcp = (F(1) / mx).astype(F)
        if rcp_ulps:
            rcp = np.nextafter(rcp, F(np.inf) if rcp_ulps > 0 else F(0)).astype(F)
        a = np.where(mx > 0, (mn * rcp).astype(F), F(0)).astype(F)
    t = (a * a).astype(F)
    p = np.full_like(a, ATAN_COEF[0])
    for c in ATAN_COEF[1:]:
        p = ((p * t).astype(F) + c).astype(F)
    r = (a * p).astype(F)
    r = np.where(ay > ax, (F(1.57079632679489661923) - r).astype(F), r)
    r = np.where(x < 0, (F(3.14159265358979323846) - r).astype(F), r)
    return np.copysign(r, y).astype(F)


def fasin_f32(s):
    s = np.asarray(s, F)
    return fatan2_f32(s, np.sqrt(((F(1) - s).astype(F) * (F(1) + s).astype(F)).astype(F)).astype(F))


def _horner(x2, coef):
    p = np.full_like(x2, coef[0])
    for c in coef[1:]:
        p = (c + (x2 * p).astype(F)).astype(F)
    return p


SIN_COEF = [F(-1.0 / 5040.0), F(1.0 / 120.0), F(-1.0 / 6.0), F(1.0)]
COS_COEF = [F(1.0 / 40320.0), F(-1.0 / 720.0), F(1.0 / 24.0), F(-0.5), F(1.0)]


def expmap_sinc_cos_f32(x):
    x = np.asarray(x, F)
    x2 = (x * x).astype(F)
    return _horner(x2, SIN_COEF), _horner(x2, COS_COEF)


def small_sincos_f32(x):
    x = np.asarray(x, F)
    sinc, c = expmap_sinc_cos_f32(x)
    return (x * sinc).astype(F), c


# ---- inputs of the probe tests (tests/test_math_gpu.py) ------------------------------------------
NEAR_MIN = np.cos(L("1e-2"))                  # |sarg| from here to the threshold: class "near"


def classify(q):
    """case class of each quaternion from its exact sarg"""
    s = np.abs(sarg_of(np.asarray(q).astype(L)))
    return np.where(s >= THRESH, "gimbal", np.where(s >= NEAR_MIN, "near", "generic"))


def gimbal_quats(rng, n):
    """n quaternions on the gimbal side: pitch +-(pi/2 - d), d uniform in [0, 3e-3], roll and yaw drawn"""
    sign, d = rng.choice([-1.0, 1.0], n).astype(L), rng.uniform(0, 3e-3, n).astype(L)
    return quat_from_euler_ld(np.stack([rng.uniform(-3.1, 3.1, n).astype(L), sign * (PI / 2 - d),
                                        rng.uniform(-3.1, 3.1, n).astype(L)], -1))


def euler_probe_inputs(dtype, n=100_000, seed=7):
    """the table, n random unit quaternions and 2,000 more on the gimbal side, rounded to `dtype`:
    (q [M, 4] dtype, class [M], longdouble reference angles of the rounded q [M, 3])"""
    rng = np.random.default_rng(seed)
    q = np.concatenate([QUAT_LD, random_unit_quats(rng, n), gimbal_quats(rng, 2000)]).astype(dtype)
    s = np.abs(sarg_of(q.astype(L)))
    assert (np.abs(s - THRESH) > MARGIN).all()
    return q, classify(q), euler_from_quat(q.astype(L))


def rpy_probe_inputs(dtype, n=100_000, seed=9):
    """angles for getQuaternionFromEuler: the table's, n uniform in (-pi, pi)^3, and 20,000 whose half
    angles straddle the pi/8 switch of quat_from_euler_fast (all three near it, within +-1e-3 relative and
    at the neighbouring floats, so one wave holds both series); rounded to `dtype`"""
    rng = np.random.default_rng(seed)
    _, ref = table(dtype)
    edge = np.float64(np.pi / 4) * (1 + rng.uniform(-1e-3, 1e-3, (20_000, 3))) * rng.choice([-1.0, 1.0], (20_000, 3))
    q4 = dtype(np.pi / 4)
    exact = np.array([[q4, q4, q4], [np.nextafter(q4, dtype(1)), q4, -q4], [q4, -np.nextafter(q4, dtype(1)), q4],
                      [np.nextafter(q4, dtype(0)), q4, q4], [0, 0, 0], [np.pi, np.pi / 2, -np.pi], [-np.pi, -np.pi / 2, np.pi]])
    rpy = np.concatenate([ref.astype(np.float64), rng.uniform(-np.pi, np.pi, (n, 3)),
                          rng.uniform(-np.pi / 4, np.pi / 4, (20_000, 3)), edge, exact.astype(np.float64)])
    return rpy.astype(dtype)


def quat_from_euler_np(rpy, dtype):
    """getQuaternionFromEuler with every operation in numpy `dtype`"""
    rpy = np.asarray(rpy, dtype)
    h = (rpy * dtype(0.5)).astype(dtype)
    s, c = np.sin(h).astype(dtype), np.cos(h).astype(dtype)
    sr, sp, sy, cr, cp, cy = s[..., 0], s[..., 1], s[..., 2], c[..., 0], c[..., 1], c[..., 2]
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                     cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], -1).astype(dtype)
