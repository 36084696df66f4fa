"""The fp64 fast transcendentals the fp64 step kernels inline (csrc/adrp_device.h namespace f64:
refined v_rcp_f64 / v_rsq_f64 / Goldschmidt sqrt, range-reduced polynomials fitted by
tools/fit_f64_poly.py) against numpy longdouble references (64-bit mantissa), through
adrp_math_probe.  Bar: 4 ulp relative (2^-50 ~ 8.9e-16) on the ranges the kernels use, 4e-16
absolute near zero crossings of atan2 / asin.  Needs an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402

L = np.longdouble
ULP4 = 2.0 ** -50


def probe(fn, x, x2=None):
    lib = _lib.load()
    inp = np.ascontiguousarray(x, np.float64) if x2 is None else np.concatenate([x, x2]).astype(np.float64)
    n = len(x)
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.empty(n, dtype=torch.float64, device="cuda")
    rc = lib.adrp_math_probe(fn, ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), n,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def rel_err(got, ref, floor=0.0):
    ref = np.asarray(ref, L)
    return np.abs(got.astype(L) - ref) / np.maximum(np.abs(ref), L(floor))


def test_constants_mirrored():
    assert (abi.MATH_RCP, abi.MATH_EXP, abi.MATH_COS_TINY) == (0, 7, 12)


def test_rcp_rsq_sqrt():
    rng = np.random.default_rng(0)
    x = np.concatenate([10.0 ** rng.uniform(-12, 12, 200000), [1.0, 2.0, 3.0, 0.1, 1e-300, 1e300]])
    assert rel_err(probe(abi.MATH_RCP, x), 1 / x.astype(L)).max() < ULP4
    assert rel_err(probe(abi.MATH_RSQ, x), 1 / np.sqrt(x.astype(L))).max() < ULP4
    assert rel_err(probe(abi.MATH_SQRT, x), np.sqrt(x.astype(L))).max() < ULP4
    z = probe(abi.MATH_SQRT, np.array([0.0, -0.0, -1.0]))
    assert z[0] == 0.0 and np.isnan(z[2])
    assert np.isinf(probe(abi.MATH_RCP, np.array([0.0]))[0])


def test_chain_variants():
    """The Bullet-step forms: sqrt of sums of squares (0 -> 0, NaN -> NaN, bit-identical to sqrt
    above 1e-300) and rcp / rsq without the non-finite fix-up (bit-identical to the checked forms on
    finite non-zero arguments)."""
    rng = np.random.default_rng(1)
    x = np.concatenate([10.0 ** rng.uniform(-12, 12, 200000), [1.0, 2.0, 3.0, 0.1, 1e-300, 1e300]])
    np.testing.assert_array_equal(probe(abi.MATH_SQRT_NN, x), probe(abi.MATH_SQRT, x))
    np.testing.assert_array_equal(probe(abi.MATH_RCP_NC, x), probe(abi.MATH_RCP, x))
    np.testing.assert_array_equal(probe(abi.MATH_RSQ_NC, x), probe(abi.MATH_RSQ, x))
    z = probe(abi.MATH_SQRT_NN, np.array([0.0, np.nan]))
    assert z[0] == 0.0 and np.isnan(z[1])


def test_sincos_tiny():
    """The short exp-map series on |x| <= 0.03 (taken when the whole wave is there)."""
    x = np.concatenate([np.linspace(-0.03, 0.03, 100001), [1e-300, -1e-12, 0.0]])
    xs = x[x != 0]
    assert rel_err(probe(abi.MATH_SIN_TINY, xs), np.sin(xs.astype(L))).max() < ULP4
    assert rel_err(probe(abi.MATH_COS_TINY, x), np.cos(x.astype(L))).max() < ULP4


def test_sincos_small():
    x = np.linspace(-np.pi / 8, np.pi / 8, 300001)
    x = x[x != 0]
    assert rel_err(probe(abi.MATH_SIN_SMALL, x), np.sin(x.astype(L))).max() < ULP4
    assert rel_err(probe(abi.MATH_COS_SMALL, x), np.cos(x.astype(L))).max() < ULP4


def test_atan2_asin():
    rng = np.random.default_rng(1)
    y = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.uniform(-3, 3, 200000), [0.0, 1.0, -1.0, 1.0, 0.0]])
    x = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.uniform(-3, 3, 200000), [1.0, 0.0, 0.0, 1.0, -1.0]])
    got = probe(abi.MATH_ATAN2, y, x)
    assert rel_err(got, np.arctan2(y.astype(L), x.astype(L)), floor=0.5).max() < ULP4
    s = np.concatenate([rng.uniform(-0.99999, 0.99999, 200000), [0.0, 0.5, -0.5]])
    assert rel_err(probe(abi.MATH_ASIN, s), np.arcsin(s.astype(L)), floor=0.5).max() < ULP4


def test_exp():
    x = np.concatenate([-np.linspace(0, 40, 200001), [-700.0, -745.5, -1e4]])
    got = probe(abi.MATH_EXP, x)
    ref = np.exp(x.astype(L))
    ok = ref > L(1e-300)
    assert rel_err(got[ok], ref[ok]).max() < ULP4
    assert got[-1] == 0.0


def test_exp_table_form():
    """the race downwash's exp (2^(j/32) table + degree-6 Taylor on |r| <= ln2/64): the same 4-ulp bar
    as exp() on x <= 0, underflow to 0 below the clamp"""
    rng = np.random.default_rng(5)
    x = np.concatenate([-np.linspace(0, 40, 200001), -rng.exponential(3.0, 200000), [-700.0, -745.5, -1e4, -0.0]])
    got = probe(abi.MATH_EXP_TAB, x)
    ref = np.exp(x.astype(L))
    ok = ref > L(1e-300)
    assert rel_err(got[ok], ref[ok]).max() < ULP4
    assert got[-2] == 0.0 and got[-1] == 1.0


def test_atan2_finite_form_matches():
    """the race Euler angles' atan2 without the non-finite fix-ups: bit-identical to atan2 on finite
    operands (zeros included)"""
    rng = np.random.default_rng(6)
    y = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.uniform(-3, 3, 200000), [0.0, 1.0, -1.0, 0.0, -0.0]])
    x = np.concatenate([rng.normal(size=200000) * 10.0 ** rng.uniform(-3, 3, 200000), [1.0, 0.0, 0.0, 0.0, -1.0]])
    np.testing.assert_array_equal(probe(abi.MATH_ATAN2_NC, y, x), probe(abi.MATH_ATAN2, y, x))


def test_non_finite_inputs():
    """NaN in -> NaN out for atan2 (fmax / fmin drop a NaN), sqrt(+inf) = +inf"""
    nan, inf = np.nan, np.inf
    got = probe(abi.MATH_ATAN2, np.array([nan, 1.0, nan, 0.0]), np.array([nan, nan, 1.0, nan]))
    assert np.isnan(got).all()
    got = probe(abi.MATH_ASIN, np.array([nan]))
    assert np.isnan(got).all()
    s = probe(abi.MATH_SQRT, np.array([inf, 0.0, -0.0, 4.0, -1.0, nan]))
    assert s[0] == inf and s[1] == 0.0 and s[3] == 2.0 and np.isnan(s[4]) and np.isnan(s[5])
    assert np.signbit(s[2])


@pytest.mark.parametrize("fn", ["sinc", "cos", "norm"])
def test_exp_map_forms_are_per_lane(fn):
    """the hover fp64 exp map picks the short series (|x| <= 0.03) and the Newton norm
    (|n2 - 1| <= 1e-9) per lane.  A lane's result must not depend on its 63 wave neighbours: the same
    inputs probed in a wave of like lanes and in waves mixed with lanes that take the other form give
    bit-identical results, and each form is accurate on its own range."""
    rng = np.random.default_rng(5)
    if fn == "norm":
        fid = abi.MATH_QUAT_INV_NORM
        near = 1.0 + rng.uniform(-1e-9, 1e-9, 64 * 64)
        far = 1.0 + rng.uniform(-1e-3, 1e-3, 64 * 64)
        far = far[np.abs(far - 1) > 1e-9]
        ref = lambda v: 1 / np.sqrt(v.astype(L))
        tol = ULP4
    else:
        fid = abi.MATH_EXPMAP_SINC if fn == "sinc" else abi.MATH_EXPMAP_COS
        near = rng.uniform(-0.03, 0.03, 64 * 64)
        far = rng.uniform(0.031, np.pi / 8, 64 * 64) * rng.choice([-1, 1], 64 * 64)
        ref = (lambda v: np.sin(v.astype(L)) / v.astype(L)) if fn == "sinc" else (lambda v: np.cos(v.astype(L)))
        tol = ULP4
    alone_near, alone_far = probe(fid, near), probe(fid, far[:len(near)])
    mixed = np.empty(2 * len(near))
    mixed[0::2], mixed[1::2] = near, far[:len(near)]      # every wave holds both forms
    got = probe(fid, mixed)
    np.testing.assert_array_equal(got[0::2], alone_near)
    np.testing.assert_array_equal(got[1::2], alone_far)
    assert rel_err(alone_near, ref(near)).max() < tol
    assert rel_err(alone_far, ref(far[:len(near)])).max() < tol


def test_race_noise_box_muller_matches_oracle():
    """the fp64 race kernels' action noise (normal_pair_f, IEEE float operations only) is the
    oracle's (oracle/race.c normal_pair_f) bit for bit on the same Philox words; both are within 2
    float ulp of the float64 libm Box-Muller"""
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    w = rng.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64)
    w = np.concatenate([w, np.array([[0xFFFFFFFF, 0], [0, 0xFFFFFFFF], [0, 0x80000000], [0x100, 0x1234567]], np.uint64)])
    bits = (w[:, 1] << np.uint64(32)) | w[:, 0]
    x = bits.view(np.float64)
    z0, z1 = probe(abi.MATH_NORMAL_Z0, x), probe(abi.MATH_NORMAL_Z1, x)
    ref = np.array([O.normal_pair(a, b) for a, b in w], np.float64)
    np.testing.assert_array_equal(z0, ref[:, 0])
    np.testing.assert_array_equal(z1, ref[:, 1])
    u1 = ((w[:, 0] >> np.uint64(8)).astype(np.float64) + 1) / 2 ** 24
    u2 = (w[:, 1] >> np.uint64(8)).astype(np.float64) / 2 ** 24
    r = np.sqrt(-2 * np.log(u1))
    assert (np.abs(z0 - r * np.cos(2 * np.pi * u2)) <= 2.5e-7 * np.maximum(r, 1e-30) + 1e-30).all()
    assert (np.abs(z1 - r * np.sin(2 * np.pi * u2)) <= 2.5e-7 * np.maximum(r, 1e-30) + 1e-30).all()


@pytest.mark.parametrize("c", [0.002, 9.8, 65535.0, 3.0, 3.16e-10, 0.2685])
def test_constant_divisor_division_is_ieee(c):
    """f64::div_c (the fp64 kernels' x / c for the wrapper's constant divisors: numpy's rates / 0.002,
    acc / 0.002 / 9.8, _compute_pwms / 65535 / 3, _thr2pwm / 3.16e-10 / 0.2685) equals the IEEE
    quotient bit for bit, signed zeros included, over 10^6 random x across 2^-60 .. 2^60"""
    rng = np.random.default_rng(int(c * 1000) % 2 ** 31)
    x = np.ldexp(1 + rng.random(1_000_000), rng.integers(-60, 61, 1_000_000)) * rng.choice([-1.0, 1.0], 1_000_000)
    x = np.concatenate([x, [0.0, -0.0, 1.0, -1.0, c, 3 * c]])
    got = probe(abi.MATH_DIVC, x, np.full_like(x, c))
    want = x / c
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def test_sincos_fast():
    """f64::sincos_fast (gate / part yaws and reset attitudes of the fp64 race kernels): within 2 ulp
    of the correctly rounded sin / cos on |x| <= 100 (relative; absolute 2^-52 near zero crossings),
    octant boundaries and signed zeros included"""
    rng = np.random.default_rng(19)
    x = np.concatenate([rng.uniform(-100, 100, 400000), rng.uniform(-4, 4, 200000),
                        np.arange(-40, 41) * np.pi / 8, [0.0, -0.0, 1e-300, np.pi, -np.pi, 0.5 * np.pi]])
    s, c = probe(abi.MATH_SIN_FAST, x), probe(abi.MATH_COS_FAST, x)
    xl = x.astype(L)
    for got, ref in ((s, np.sin(xl)), (c, np.cos(xl))):
        err = np.abs(got.astype(L) - ref)
        assert (err <= np.maximum(np.abs(ref) * L(2.0 ** -51), L(2.0 ** -52))).all(), float(err.max())
    assert s[-6] == 0.0 and c[-6] == 1.0


def test_fdiv_rcp_is_ieee_float_division():
    """f64::fdiv_rcp (the fp64 race firmware's float divisions, race_kernel.h mellinger_fw): rounding
    x * rcp(y) to float is the IEEE float x / y bit for bit.  4M quotients: random bit patterns over
    the whole normal range (both signs), quotients near float rounding boundaries (y a float just off
    a power of two, x with all-ones / alternating significands), the firmware's own scales (norms of
    target / y_des vectors, D terms by dt = 0.002f)"""
    rng = np.random.default_rng(23)
    n = 1 << 20

    def rand_f32(k, lo_exp=-60, hi_exp=60):
        m = rng.integers(0, 1 << 23, k, dtype=np.uint32)
        e = rng.integers(127 + lo_exp, 127 + hi_exp, k).astype(np.uint32)
        s = rng.integers(0, 2, k, dtype=np.uint32) << 31
        return (s | (e << 23) | m).view(np.float32)
    xs = [rand_f32(n), rand_f32(n, -3, 3), rng.uniform(-3, 3, n).astype(np.float32)]
    ys = [rand_f32(n), rand_f32(n, -3, 3), rng.uniform(0.05, 3, n).astype(np.float32)]
    # adversarial: y = 2^k (1 + j ulp) with small j, x with long runs of ones in the significand
    j = rng.integers(1, 64, n).astype(np.uint32)
    y_adv = ((np.uint32(127) << 23) + j).view(np.float32) * np.float32(2.0) ** rng.integers(-4, 4, n).astype(np.float32)
    x_adv = ((np.uint32(127) << 23) | (np.uint32((1 << 23) - 1) ^ rng.integers(0, 8, n, dtype=np.uint32))).view(np.float32)
    xs.append(x_adv)
    ys.append(y_adv)
    xs.append(rng.uniform(-50, 50, n).astype(np.float32))
    ys.append(np.full(n, np.float32(1.0) / np.float32(500), np.float32))
    for x, y in zip(xs, ys):
        got = probe(abi.MATH_FDIV_RCP, x.astype(np.float64), y.astype(np.float64)).astype(np.float32)
        ref = x / y
        bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
        assert len(bad) == 0, f"{len(bad)} quotients differ, e.g. {x[bad[:4]]} / {y[bad[:4]]}: {got[bad[:4]]} vs {ref[bad[:4]]}"


# ---- the attitude forms and the fp32 fast forms (adrp_math_probe_v) -------------------------------
# The probe TU compiles with the race TUs' contraction mode, so these results stand for the race
# kernels' bits; the hover TUs' are checked through env.step (tests/test_attitude_edges_gpu.py).
import attitude_cases as AC  # noqa: E402

F32_ULP = 2.0 ** -23
PREC = {"fp32": (0, np.float32), "fp64": (1, np.float64)}


def probe_v(fn, precision, *planes):
    """planes: k_in arrays of n values -> [k_out, n] float64 (float results widened exactly)"""
    lib = _lib.load()
    k_in, k_out = abi.MATHV_PLANES[fn]
    assert len(planes) == k_in
    inp = np.ascontiguousarray(np.stack([np.asarray(p, np.float64) for p in planes]))
    n = inp.shape[1]
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.empty((k_out, n), dtype=torch.float64, device="cuda")
    rc = lib.adrp_math_probe_v(fn, precision, ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), n,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_fatan2_float():
    """fp32 fatan2_ against longdouble.  5e-7 rad absolute over all operand pairs (emulated floor 2.9e-7,
    3.4e-7 with the reciprocal one ulp off: tests/test_attitude_edges.py).  Relative for |y / x| <= 1e-3:
    a first proposal of 2.5e-7 assumed one IEEE division (6.8e-8); the kernel multiplies by v_rcp_f32, and the
    emulation with that reciprocal one ulp off reaches 2.72e-7, which contradicts 2.5e-7, so the bar is
    the emulation's figure, 2.8e-7.  Seams: fatan2_(+-0, -1) = +-pi, fatan2_(0, 0) = 0, |result| <= pi."""
    rng = np.random.default_rng(41)
    n = 200_000
    y = (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1, 1], n)).astype(np.float32)
    x = (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1, 1], n)).astype(np.float32)
    ys = (x * 10.0 ** rng.uniform(-9, -3, n)).astype(np.float32)        # small angles, both seams
    y, x = np.concatenate([y, ys, rng.normal(size=n).astype(np.float32)]), np.concatenate([x, x, rng.normal(size=n).astype(np.float32)])
    got = probe_v(abi.MATHV_FATAN2, 0, y, x)[0]
    ref = np.arctan2(y.astype(L), x.astype(L))
    err = np.abs(got.astype(L) - ref)
    small = (np.abs(y.astype(L) / x.astype(L)) <= 1e-3) & (x > 0)
    print("fatan2_ float: abs", float(err.max()), "rel small", float((err[small] / np.abs(ref[small])).max()))
    assert err.max() <= 5e-7
    assert (err[small] / np.abs(ref[small])).max() <= 2.8e-7
    assert (np.abs(got) <= float(np.float32(np.pi))).all()
    pi32 = float(np.float32(np.pi))
    seam = probe_v(abi.MATHV_FATAN2, 0, np.array([0.0, -0.0, 0.0, -0.0, 0.0, 1.0, -1.0]),
                   np.array([-1.0, -1.0, 0.0, 0.0, 1.0, 0.0, 0.0]))[0]
    assert seam[0] == pi32 and seam[1] == -pi32 and seam[2] == 0 and seam[3] == 0 and seam[4] == 0
    assert np.signbit(seam[1]) and seam[5] == float(np.float32(np.pi / 2)) and seam[6] == -seam[5]


def test_fasin_float():
    """fp32 fasin_ on |s| <= 0.99998 (the generic branch's range): 5e-7 rad absolute (emulated floor 2.1e-7)"""
    rng = np.random.default_rng(42)
    s = np.concatenate([rng.uniform(-0.99998, 0.99998, 300_000), 1 - 10.0 ** rng.uniform(-4.69, -1, 50_000),
                        [0.0, 0.5, -0.5, 0.99998, -0.99998]]).astype(np.float32)
    s = s[np.abs(s) <= np.float32(0.99998)]
    err = np.abs(probe_v(abi.MATHV_FASIN, 0, s)[0].astype(L) - np.arcsin(s.astype(L)))
    print("fasin_ float: abs", float(err.max()))
    assert err.max() <= 5e-7


def test_small_series_float():
    """fp32 small_sincos / expmap_sinc_cos on |x| <= pi/8: 4 float ulp relative (emulated floor < 1 ulp)"""
    x = np.concatenate([np.linspace(-np.pi / 8, np.pi / 8, 300_001), [1e-30, -1e-12, 0.0]]).astype(np.float32)
    x = x[np.abs(x) <= np.float32(np.pi / 8)]
    xl = x.astype(L)
    s, c = probe_v(abi.MATHV_SMALL_SINCOS, 0, x)
    sinc, c2 = probe_v(abi.MATHV_EXPMAP_SINC_COS, 0, x)
    nz = x != 0
    e_sin = rel_err(s[nz], np.sin(xl[nz])).max() / F32_ULP
    e_cos = max(rel_err(c, np.cos(xl)).max(), rel_err(c2, np.cos(xl)).max()) / F32_ULP
    e_sinc = rel_err(sinc[nz], np.sin(xl[nz]) / xl[nz]).max() / F32_ULP
    print("small series float, ulp: sin", float(e_sin), "cos", float(e_cos), "sinc", float(e_sinc))
    assert max(e_sin, e_cos, e_sinc) <= 4
    assert s[~nz][0] == 0 and c[~nz][0] == 1 and sinc[~nz][0] == 1


def test_quat_inv_norm_float():
    """fp32 quat_inv_norm (v_rsq_f32): 2 float ulp"""
    rng = np.random.default_rng(43)
    n2 = np.concatenate([1 + rng.uniform(-1e-3, 1e-3, 100_000), 10.0 ** rng.uniform(-6, 6, 100_000), [1.0, 0.25, 4.0]]).astype(np.float32)
    err = rel_err(probe_v(abi.MATHV_QUAT_INV_NORM, 0, n2)[0], 1 / np.sqrt(n2.astype(L))).max() / F32_ULP
    print("quat_inv_norm float, ulp:", float(err))
    assert err <= 2


def test_fexp_float():
    """fp32 fexp_ = v_exp_f32(x log2 e) on [-30, 0]: relative 2.5e-7 + 1.5e-7 |x| (the rounding of
    x log2 e scales with |x|, plus one ulp of v_exp_f32); below -87 the result underflows into [0, 2^-125]"""
    rng = np.random.default_rng(44)
    x = np.concatenate([-np.linspace(0, 30, 200_001), -rng.exponential(3.0, 100_000).clip(0, 30), [-0.0]]).astype(np.float32)
    got = probe_v(abi.MATHV_FEXP, 0, x)[0]
    rel = rel_err(got, np.exp(x.astype(L)))
    bar = 2.5e-7 + 1.5e-7 * np.abs(x.astype(np.float64))
    print("fexp_ float: worst rel / bar", float((rel / bar).max()), "rel at 0..1", float(rel[np.abs(x) <= 1].max()))
    assert (rel <= bar).all()
    assert got[-1] == 1.0
    under = probe_v(abi.MATHV_FEXP, 0, np.array([-87.5, -88.0, -100.0, -1000.0, -3e38], np.float32))[0]
    assert (under >= 0).all() and (under <= 2.0 ** -125).all()


EULER_FORMS = {"euler_xyz": abi.MATHV_EULER_XYZ, "euler_xyz_fast": abi.MATHV_EULER_XYZ_FAST,
               "euler_xyz_fast_u": abi.MATHV_EULER_XYZ_FAST_U}


@pytest.fixture(scope="module")
def euler_inputs():
    """(q, class, longdouble reference, error of the same formula in numpy's type) per precision, computed once"""
    out = {}
    for name, (_, dt) in PREC.items():
        q, cls, ref = AC.euler_probe_inputs(dt)
        own = AC.rpy_err(AC.euler_from_quat(q, dt), ref).max(-1)
        out[name] = (q, cls, ref, own)
    return out


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("form", list(EULER_FORMS))
def test_euler_forms(euler_inputs, form, precision):
    """euler_xyz / euler_xyz_fast / euler_xyz_fast_u on the constructed table (tests/attitude_cases.py:
    gimbal branches, the +-pi seams, -q), 100k random unit quaternions and 2k on the gimbal side, against
    the longdouble getEulerFromQuaternion of the same (rounded) quaternion, roll and yaw on the circle.
    Bar per case class: 4 x the error of the same formula evaluated in numpy's float64 / float32 on these
    inputs (the margin covers the 4-ulp f64::atan2 / the fp32 fatan2_ against libm):

        class                                   float64 formula   bar        float32 formula   bar
        generic  (|sin pitch| <  cos 1e-2)      8.5e-15           3.4e-14    4.9e-6            2.0e-5
        near     (cos 1e-2 <= |sin pitch|)      1.1e-14           4.2e-14    9.0e-6            3.6e-5
        gimbal   (|sin pitch| >= 0.99999)       6.3e-16           2.5e-15    5.5e-7            2.2e-6

    (rad; the generic figures are set by the random quaternions closest to the near class, where the
    atan2 arguments are small differences).  Gimbal rows are exactly (0, +-pi/2, .)."""
    prec, dt = PREC[precision]
    q, cls, ref, own = euler_inputs[precision]
    got = probe_v(EULER_FORMS[form], prec, *(q[:, k] for k in range(4))).T
    err = AC.rpy_err(got, ref).max(-1)
    for c in AC.CLASSES:
        m = cls == c
        assert m.sum() >= 12
        bar = 4 * float(own[m].max())
        print(f"{form} {precision} {c}: {float(err[m].max()):.3e} (formula {float(own[m].max()):.3e}, bar {bar:.3e})")
        assert err[m].max() <= bar, c
    g = cls == "gimbal"
    assert (got[g, 0] == 0).all()
    np.testing.assert_array_equal(np.abs(got[g, 1]), float(dt(np.pi / 2)))
    np.testing.assert_array_equal(np.sign(got[g, 1]), np.sign(AC.sarg_of(q[g].astype(L)).astype(np.float64)))
    assert np.isfinite(got).all()
    if precision == "fp32":        # float angles stay inside [-pi, pi] (generic) as floats
        assert (np.abs(got[~g]) <= float(np.float32(np.pi))).all()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("form", ["quat_from_euler", "quat_from_euler_fast"])
def test_quat_from_euler_forms(form, precision):
    """getQuaternionFromEuler forms against longdouble on the table's angles, 100k uniform in (-pi, pi)^3 and
    40k with half angles inside / straddling the pi/8 series switch of quat_from_euler_fast.  Bar: 4 x the
    error of the same formula in numpy's type on these inputs (float64 2.7e-16 -> 1.1e-15, float32
    1.5e-7 -> 6.0e-7, per component); unit norm to the same bar."""
    prec, dt = PREC[precision]
    rpy = AC.rpy_probe_inputs(dt)
    want = AC.quat_from_euler_ld(rpy.astype(L))
    own = float(np.abs(AC.quat_from_euler_np(rpy, dt).astype(L) - want).max())
    fn = abi.MATHV_QUAT_FROM_EULER if form == "quat_from_euler" else abi.MATHV_QUAT_FROM_EULER_FAST
    got = probe_v(fn, prec, *(rpy[:, k] for k in range(3))).T
    err = np.abs(got.astype(L) - want).max(-1)
    inside = (np.abs(rpy.astype(np.float64)) <= 2 * 0.39269908169872414).all(-1)
    assert inside.sum() > 10_000 and (~inside).sum() > 10_000
    print(f"{form} {precision}: small series {float(err[inside].max()):.3e}, else {float(err[~inside].max()):.3e} "
          f"(formula {own:.3e}, bar {4 * own:.3e})")
    assert err.max() <= 4 * own
    assert np.abs((got.astype(L) ** 2).sum(-1) - 1).max() <= 4 * 4 * own      # |q|^2 - 1 = 2 q.e, |e|_2 <= 2 bar


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_euler_vote_is_per_lane(precision):
    """euler_xyz_fast_u takes euler_xyz_fast for the whole wave when any lane is in gimbal lock.  A
    lane's angles must not depend on its wave mates: 4,096 generic quaternions probed alone (no wave
    votes) and interleaved with 4,096 gimbal-side ones (every wave votes) give bit-identical results,
    and so do the gimbal lanes alone and interleaved; both equal the unvoted euler_xyz_fast (before
    the Euler arguments' contraction was pinned, csrc/adrp_device.h euler_args, two inlined copies of
    euler_xyz_fast in this translation unit differed in 2.4 % (fp64, <= 19 ulp) / 4.8 % (fp32, <= 47 ulp)
    of these angles)."""
    prec, dt = PREC[precision]
    rng = np.random.default_rng(47)
    n = 4096
    gen = np.concatenate([AC.QUAT_LD[AC.SIDE == "generic"], AC.random_unit_quats(rng, 2 * n)])
    gen = gen[AC.classify(gen.astype(dt)) != "gimbal"][:n].astype(dt)
    gim = np.concatenate([AC.QUAT_LD[AC.SIDE == "gimbal"], AC.gimbal_quats(rng, n)])[:n].astype(dt)
    assert len(gen) == n and len(gim) == n
    assert (np.abs(AC.sarg_of(gen, dt)) < dt(0.99999)).all() and (np.abs(AC.sarg_of(gim, dt)) >= dt(0.99999)).all()
    fu = abi.MATHV_EULER_XYZ_FAST_U

    def run(fn, q):
        return probe_v(fn, prec, *(q[:, k] for k in range(4))).T
    alone_gen, alone_gim = run(fu, gen), run(fu, gim)
    mixed = np.empty((2 * n, 4), dt)
    mixed[0::2], mixed[1::2] = gen, gim
    got = run(fu, mixed)
    np.testing.assert_array_equal(got[0::2].view(np.uint64), alone_gen.view(np.uint64))
    np.testing.assert_array_equal(got[1::2].view(np.uint64), alone_gim.view(np.uint64))
    one = mixed.copy()                       # a single gimbal lane per wave
    one[1::2] = gen[::-1]
    one[63::64] = gim[: len(one[63::64])]
    got1 = run(fu, one)
    np.testing.assert_array_equal(got1[0::2].view(np.uint64), alone_gen.view(np.uint64))
    np.testing.assert_array_equal(run(abi.MATHV_EULER_XYZ_FAST, mixed).view(np.uint64), got.view(np.uint64))
    assert (alone_gim[:, 0] == 0).all() and (alone_gen[:, 0] != 0).any()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_clamp100_wv(precision):
    """clamp100_wv (btClamp of the six coordinate velocities): +-100 and the neighbouring values either
    side, in every component; fp64 lets NaN through (btClamp's comparisons are false); a lane's result does
    not depend on whether a wave mate exceeds 100 (the fp64 form's wave-uniform guard)."""
    prec, dt = PREC[precision]
    hundred = dt(100)
    edge = np.array([hundred, np.nextafter(hundred, dt(0)), np.nextafter(hundred, dt(1000)), dt(250), dt(1e30)], dt)
    edge = np.concatenate([edge, -edge, [0.0, -0.0, 1.0, 99.0]]).astype(dt)
    rng = np.random.default_rng(48)
    n = 4096
    inside = rng.uniform(-100, 100, (6, n)).astype(dt)
    inside[:, : len(edge)] = np.where(np.abs(edge) <= 100, edge, 0)[None]
    outside = rng.uniform(-300, 300, (6, n)).astype(dt)
    for k in range(6):                         # each edge value in each component, the others inside
        outside[k, k * len(edge):(k + 1) * len(edge)] = edge
    outside[0, 6 * len(edge):] = 100 + np.abs(outside[0, 6 * len(edge):])   # every such lane exceeds
    alone_in, alone_out = probe_v(abi.MATHV_CLAMP100_WV, prec, *inside), probe_v(abi.MATHV_CLAMP100_WV, prec, *outside)
    np.testing.assert_array_equal(alone_in, inside.astype(np.float64))
    np.testing.assert_array_equal(alone_out, np.clip(outside, dt(-100), dt(100)).astype(np.float64))
    mixed = np.empty((6, 2 * n), dt)
    mixed[:, 0::2], mixed[:, 1::2] = inside, outside
    got = probe_v(abi.MATHV_CLAMP100_WV, prec, *mixed)
    np.testing.assert_array_equal(got[:, 0::2].view(np.uint64), alone_in.view(np.uint64))
    np.testing.assert_array_equal(got[:, 1::2].view(np.uint64), alone_out.view(np.uint64))
    if precision == "fp64":
        v = np.array([[np.nan, 1.0, 250.0, -250.0, 100.0, -100.0]] * 3).T.copy()      # [6, 3]
        v[:, 1] = [1.0, np.nan, 2.0, 3.0, 4.0, 5.0]                                    # NaN with no lane above 100
        v[:, 2] = 50.0
        out = probe_v(abi.MATHV_CLAMP100_WV, 1, *v)
        assert np.isnan(out[0, 0]) and np.isnan(out[1, 1])
        np.testing.assert_array_equal(out[1:, 0], [1.0, 100.0, -100.0, 100.0, -100.0])
        np.testing.assert_array_equal(out[[0, 2, 3, 4, 5], 1], [1.0, 2.0, 3.0, 4.0, 5.0])
