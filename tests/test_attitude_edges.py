"""Attitude edges without a GPU: the table of constructed attitudes (tests/attitude_cases.py) keeps
its margin to the gimbal threshold in every real type, the oracle's Euler / quaternion conversions
agree with the longdouble forms on it, and a numpy float32 emulation of the fp32 fast forms
(fatan2_, fasin_, small_sincos, expmap_sinc_cos of csrc/adrp_device.h; IEEE 1 / x in place of
v_rcp_f32) records the error floors the GPU bars of tests/test_math_gpu.py rest on.

Measured floors (this file asserts them with a few percent of headroom):
  fatan2_   2M log-spaced operand pairs    2.86e-7 rad absolute; 3.36e-7 with the reciprocal moved
            one ulp either way
            |y / x| <= 1e-3                1.58e-7 relative; 2.72e-7 with the reciprocal moved one ulp.
            (A single IEEE division mn / mx gives 6.8e-8; the kernel multiplies by a reciprocal, two
            roundings, so the probe's relative bar is 2.8e-7, not 2.5e-7: test_math_gpu.py.)
  fasin_    |s| <= 0.99999                 2.09e-7 rad absolute
  small_sincos / expmap_sinc_cos, |x| <= pi/8   0.75 / 0.35 / 0.30 float ulp (sin, cos, sinc)
"""
import numpy as np
import pytest

import attitude_cases as A
from oracle import oracle as O

L = np.longdouble
F = np.float32
HALF_STEP_BAR = 0.5e-4        # half the fp32 step-parity bar (1e-4 relative, 2-norm of the rpy block)


def test_table_sides_and_margin():
    """every case is on its stated side of the gimbal threshold and at least 4e-6 from it, as a
    longdouble, a float64 and a float32 quaternion alike; -q follows q; both signs of w occur"""
    assert len(A.CASES) == len(set(A.NAMES)) and len(A.CASES) % 2 == 0
    np.testing.assert_array_equal(A.QUAT_LD[1::2], -A.QUAT_LD[0::2])
    s = np.abs(A.sarg_of(A.QUAT_LD))
    assert (s[A.SIDE == "generic"] <= A.GENERIC_MAX).all()
    assert (s[A.SIDE == "gimbal"] >= A.GIMBAL_MIN).all()
    for dt in (L, np.float64, np.float32):
        q = A.QUAT_LD.astype(dt)
        assert np.abs((q.astype(L) ** 2).sum(-1) - 1).max() < 4 * np.finfo(dt).eps
        for prec in (L, dt):                             # the exact sarg and the one the kernel's type computes
            sr = np.abs(A.sarg_of(q.astype(prec), prec).astype(L))
            assert (np.abs(sr - A.THRESH) > A.MARGIN).all(), dt
            np.testing.assert_array_equal(sr >= A.THRESH, A.SIDE == "gimbal")
    assert (A.QUAT_LD[:, 3] < 0).sum() > 40 and (A.QUAT_LD[:, 3] > 0).sum() > 40
    for cls in A.CLASSES:
        assert len(A.select(cls=cls)) >= 12
    assert sum(A.FP32_DROPPABLE in n for n in A.NAMES) == 12


def test_reference_branches_and_round_trip():
    """the longdouble reference itself: gimbal rows are (0, +-pi/2, 2 atan2), generic rows invert the
    longdouble getQuaternionFromEuler (up to the sign of q)"""
    ref = A.euler_from_quat(A.QUAT_LD)
    g = A.SIDE == "gimbal"
    assert (ref[g, 0] == 0).all() and (np.abs(ref[g, 1]) == A.PI / 2).all()
    back = A.quat_from_euler_ld(ref[~g])
    dot = np.abs((back * A.QUAT_LD[~g]).sum(-1))
    # near pitch +-pi/2 the angles are ill-conditioned but the rotation is not
    assert np.abs(dot - 1).max() < 1e-17
    # q and -q are one rotation: the same angles to longdouble rounding
    assert A.rpy_err(ref[0::2], ref[1::2]).max() < 1e-15


def test_oracle_euler_from_quat():
    """orc_euler_from_quat (libm double) on the float64 table against the longdouble form: within
    4 x the numpy float64 evaluation's own error per case class, floor 4 ulp of pi"""
    q, ref = A.table(np.float64)
    got = np.array([O.euler_from_quat(r) for r in q])
    err = A.rpy_err(got, ref).max(-1)
    f64 = A.rpy_err(A.euler_from_quat(q, np.float64), ref).max(-1)
    for cls in A.CLASSES:
        m = A.CLASS == cls
        bar = max(4 * float(f64[m].max()), 4 * 2.0 ** -52 * np.pi)
        print(f"orc_euler_from_quat {cls}: {float(err[m].max()):.3e} (float64 formula {float(f64[m].max()):.3e}, bar {bar:.3e})")
        assert err[m].max() <= bar, cls
    gim = A.SIDE == "gimbal"
    assert (got[gim, 0] == 0).all() and (np.abs(got[gim, 1]) == np.pi / 2).all()


def test_oracle_quat_from_euler():
    """orc_quat_from_euler against the longdouble form: each component is a sum of two products of
    three correctly rounded-ish sin / cos values, 8 double roundings of values <= 1: 1e-15 absolute"""
    rng = np.random.default_rng(3)
    _, ref = A.table(np.float64)
    rpy = np.concatenate([ref.astype(np.float64), rng.uniform(-np.pi, np.pi, (2000, 3)),
                          rng.uniform(-np.pi / 4, np.pi / 4, (2000, 3)) * (1 + 1e-3)])
    got = np.array([O.quat_from_euler(r) for r in rpy])
    want = A.quat_from_euler_ld(rpy.astype(L))
    assert np.abs(got.astype(L) - want).max() < 1e-15
    assert np.abs((got ** 2).sum(-1) - 1).max() < 1e-15


def test_fatan2_emulation_floor():
    rng = np.random.default_rng(1)
    n = 2_000_000
    y = (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1, 1], n)).astype(F)
    x = (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1, 1], n)).astype(F)
    ref = np.arctan2(y.astype(L), x.astype(L))
    small = np.abs(y.astype(L) / x.astype(L)) <= 1e-3
    worst_abs, worst_rel = {}, {}
    for u in (0, 1, -1):
        err = np.abs(A.fatan2_f32(y, x, u).astype(L) - ref)
        worst_abs[u] = float(err.max())
        worst_rel[u] = float((err[small] / np.abs(ref[small])).max())
    print("fatan2_ emulation: abs", worst_abs, "rel(|y/x| <= 1e-3)", worst_rel)
    assert worst_abs[0] <= 2.9e-7
    assert max(worst_abs.values()) <= 3.5e-7            # + one-ulp v_sqrt / contraction -> GPU bar 5e-7
    assert worst_rel[0] <= 1.65e-7
    # the reciprocal's ulp enters the small-angle result whole (r = mn * rcp(mx) * p, p ~ 1): the
    # 2.5e-7 relative bar has no room for it, 2.8e-7 has
    assert 2.5e-7 < max(worst_rel.values()) <= 2.8e-7
    # signs and seams of the emulated form (the GPU test asserts the same of the kernel's)
    pz, nz, one = F(0.0), F(-0.0), F(1.0)
    assert A.fatan2_f32(pz, -one) == F(np.pi) and A.fatan2_f32(nz, -one) == -F(np.pi)
    assert A.fatan2_f32(pz, pz) == 0 and A.fatan2_f32(nz, nz) == 0
    g = A.fatan2_f32(y, x)
    assert (np.abs(g) <= F(np.pi)).all()


def test_fasin_emulation_floor():
    rng = np.random.default_rng(2)
    s = np.concatenate([rng.uniform(-0.99999, 0.99999, 2_000_000), [0.99999, -0.99999, 0.99998, 0.0]]).astype(F)
    s = s[np.abs(s) <= F(0.99999)]
    err = float(np.abs(A.fasin_f32(s).astype(L) - np.arcsin(s.astype(L))).max())
    print("fasin_ emulation: abs", err)
    assert err <= 2.2e-7                                 # + one-ulp v_sqrt, v_rcp -> GPU bar 5e-7


def test_small_series_emulation_floor():
    x = np.linspace(-np.pi / 8, np.pi / 8, 400001).astype(F)
    x = x[x != 0]
    xl = x.astype(L)
    sn, cs = A.small_sincos_f32(x)
    sinc, cs2 = A.expmap_sinc_cos_f32(x)
    np.testing.assert_array_equal(cs, cs2)
    ulp = L(2.0) ** -23
    e_sin = float((np.abs(sn.astype(L) - np.sin(xl)) / np.abs(np.sin(xl))).max() / ulp)
    e_cos = float((np.abs(cs.astype(L) - np.cos(xl)) / np.cos(xl)).max() / ulp)
    e_sinc = float((np.abs(sinc.astype(L) - np.sin(xl) / xl) / (np.sin(xl) / xl)).max() / ulp)
    print("small series emulation, float ulp: sin", e_sin, "cos", e_cos, "sinc", e_sinc)
    assert max(e_sin, e_cos, e_sinc) <= 1.0              # GPU bar: 4 ulp


def test_fp32_formula_within_half_the_step_bar():
    """the condition for the fp32 env tests (test_attitude_edges_gpu.py): getEulerFromQuaternion
    evaluated in float32 from the float32 quaternion stays within half the step-parity bar of the
    longdouble angles at every generic point, so an fp32 kernel that is right has the other half for
    its fast atan2 / asin.  It holds at pitch = +-(pi/2 - 6.5e-3) too (worst 3.7e-6 of 5e-5): no
    case is dropped from the fp32 tests."""
    q, ref = A.table(np.float32)
    rel = A.rpy_rel_err(A.euler_from_quat(q, np.float32), ref)
    gen = A.SIDE == "generic"
    worst = int(np.argmax(np.where(gen, rel, 0)))
    print(f"float32 formula, generic side: worst {float(rel[worst]):.3e} at {A.NAMES[worst]}")
    assert rel[gen].max() <= HALF_STEP_BAR
    assert rel[~gen].max() <= HALF_STEP_BAR
    # the fast forms' emulation on the same points
    x, y, z, w = (q[:, k] for k in range(4))
    two = F(2)
    fast = np.stack([A.fatan2_f32(two * (y * z + w * x), w * w - x * x - y * y + z * z),
                     A.fasin_f32(np.clip(F(-2) * (x * z - w * y), F(-1), F(1))),
                     A.fatan2_f32(two * (x * y + w * z), w * w + x * x - y * y - z * z)], -1)
    assert A.rpy_rel_err(fast[gen], ref[gen]).max() <= HALF_STEP_BAR
