"""Stand-alone DSLPIDControl, the checks that need no GPU: the numpy restatement the GPU tests compare with
(tests/dslpid_reference.py) reproduces the reference's own outputs (tests/golden/dslpid_golden.npz, both parts,
and pid_golden.npz's dsl_*) at 1e-9; the header declares and the library exports the new entry points; the
argument errors come back before any device call; the Python class refuses what the reference refuses.

Bar (tests/test_hover_gpu.py): per vector |x - x_ref| <= rtol * max(|x_ref|, floor), 2-norms; floors 1.0 for the
RPMs (``last_rpm``), 1e-3 for pos_e, yaw_e and the three controller state vectors.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import dslpid_reference as ref
from gym_pybullet_adrp_amd.utils import abi
from gym_pybullet_adrp_amd.utils.enums import DroneModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adrp.h")
RTOL = 1e-9
NEW_SYMBOLS = ["adrp_dslpid_default_params", "adrp_dslpid_create", "adrp_dslpid_destroy", "adrp_dslpid_reset",
               "adrp_dslpid_set_gains", "adrp_dslpid_get_state", "adrp_dslpid_set_state", "adrp_dslpid_compute",
               "adrp_dslpid_compute_env"]


@pytest.fixture(scope="module")
def fx():
    return ref.load()


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_adrp_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("tag", ["x", "p"])
def test_restatement_reproduces_sequences(fx, tag):
    cin = fx[f"{tag}_in"]
    S, T = cin.shape[:2]
    assert (S, T) == (24, 10) and float(fx["dt"]) == 1 / 48
    assert fx[f"{tag}_GRAVITY"] == 9.8 * ref.MASS[ref.MIXER_OF[tag]] and fx[f"{tag}_KF"] == ref.KF
    np.testing.assert_array_equal(fx[f"{tag}_MIXER"], ref.MIXERS[ref.MIXER_OF[tag]])
    flags = fx[f"{tag}_flags"]
    assert all(flags[..., k].any() for k in range(7)) and (flags[..., 5] & 1).any() and (flags[..., 5] & 2).any()
    assert (flags[..., 4] == 0).any()
    for name, sel, gains in (("default", slice(0, 16), None), ("gains", slice(16, 24), ref.fixture_gains(fx))):
        c = ref.Controller(cin[sel].shape[0], ref.MIXER_OF[tag], gains=gains)
        c.state = fx[f"{tag}_st0"][sel].copy()
        for t in range(T):
            i = cin[sel, t]
            rpm, pos_e, yaw_e = c.compute(1 / 48, i[:, 0:3], i[:, 3:7], i[:, 7:10], i[:, 10:13], i[:, 13:16], i[:, 16:19], i[:, 19:22])
            ref.assert_outputs(rpm, pos_e, yaw_e, c.state, fx[f"{tag}_rpm"][sel, t], fx[f"{tag}_pos_e"][sel, t],
                               fx[f"{tag}_yaw_e"][sel, t], fx[f"{tag}_state"][sel, t], RTOL, f"{tag} {name} t={t} ")


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("tag", ["x", "p"])
def test_restatement_reproduces_pid_loop(fx, tag, N):
    case = f"loop_{tag}{N}"
    T = fx[f"{case}_obs"].shape[0]
    assert T == 24 and fx[f"{case}_obs"][..., 2].min() > 0.3
    c = ref.Controller(N, ref.MIXER_OF[tag])
    for t in range(T):
        rows = fx[f"{case}_obs"][t]
        c.state = ref.loop_ctl_before(fx, case, t)
        rpm, pos_e, yaw_e = c.compute(1 / 48, rows[:, 0:3], rows[:, 3:7], rows[:, 10:13], fx[f"{case}_tpos"][t], fx[f"{case}_trpy"])
        ref.assert_outputs(rpm, pos_e, yaw_e, c.state, fx[f"{case}_rpm"][t], fx[f"{case}_pos_e"][t], fx[f"{case}_yaw_e"][t],
                           fx[f"{case}_ctl"][t], RTOL, f"{case} t={t} ")


def test_restatement_reproduces_pid_golden():
    pg = np.load(os.path.join(ROOT, "tests", "golden", "pid_golden.npz"))
    cin, want_rpm, want_st = pg["dsl_in"], pg["dsl_rpm"], pg["dsl_state"]
    S, T = cin.shape[:2]
    c = ref.Controller(S, "cf2x")
    for t in range(T):
        i = cin[:, t]
        rpm, _, _ = c.compute(1 / 30, i[:, 0:3], i[:, 3:7], i[:, 7:10], i[:, 10:13], i[:, 13:16], i[:, 16:19])
        assert ref.vec_err(rpm, want_rpm[:, t], 1.0).max() <= RTOL
        for k, g in enumerate(ref.STATE_GROUPS):
            assert ref.vec_err(c.state[:, 3 * k:3 * k + 3], want_st[:, t, 3 * k:3 * k + 3], 1e-3).max() <= RTOL, (g, t)


def test_header_declares_and_library_exports(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(adrp_[a-z_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+ADRP_ABI_VERSION\s+2\b", open(HEADER).read()) and lib.adrp_abi_version() == 2
    p = abi.AdrpDslpidParams()
    assert lib.adrp_dslpid_default_params(abi.DSLPID_CF2X, ctypes.byref(p)) == 0
    assert p.struct_size == ctypes.sizeof(abi.AdrpDslpidParams)
    for model, key in ((abi.DSLPID_CF2X, "cf2x"), (abi.DSLPID_CF2P, "cf2p")):
        assert lib.adrp_dslpid_default_params(model, ctypes.byref(p)) == 0
        np.testing.assert_array_equal(np.array(abi.to_list(p.mixer)), ref.MIXERS[key])
        assert p.gravity == 9.8 * ref.MASS[key] and p.kf == ref.KF
        for f, v in ref.DEFAULT_GAINS.items():
            assert abi.to_list(getattr(p, f)) == v
        assert (p.pwm2rpm_scale, p.pwm2rpm_const, p.min_pwm, p.max_pwm) == (ref.PWM2RPM_SCALE, ref.PWM2RPM_CONST, ref.MIN_PWM, ref.MAX_PWM)
    assert lib.adrp_dslpid_default_params(2, ctypes.byref(p)) == abi.ERR_INVALID


def test_argument_errors_before_device(lib):
    p = abi.AdrpDslpidParams()
    assert lib.adrp_dslpid_default_params(abi.DSLPID_CF2X, ctypes.byref(p)) == 0
    for rows, precision, size, msg in ((0, 1, None, b"rows must be > 0"), (-3, 0, None, b"rows must be > 0"),
                                       (4, 2, None, b"precision must be 0 or 1"), (4, -1, None, b"precision must be 0 or 1"),
                                       (4, 1, 12, b"struct_size mismatch")):
        q = abi.AdrpDslpidParams()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(p))
        if size is not None:
            q.struct_size = size
        h = ctypes.c_void_p()
        assert lib.adrp_dslpid_create(rows, precision, ctypes.byref(q), 0, ctypes.byref(h)) == abi.ERR_INVALID
        assert msg in lib.adrp_last_error(None), lib.adrp_last_error(None)
        assert not h.value
    # control_timestep is checked first, so the refusal needs no controller (none can exist without a GPU)
    for dt in (0.0, -1 / 48, float("nan")):
        assert lib.adrp_dslpid_compute(None, dt, None, None, None, 0, 0, None, None, None, None, None, None, None, None) == abi.ERR_INVALID
        assert b"control_timestep must be > 0" in lib.adrp_last_error(None)
        assert lib.adrp_dslpid_compute_env(None, dt, None, None, None, None, None, None, None, None, None) == abi.ERR_INVALID
        assert b"control_timestep must be > 0" in lib.adrp_last_error(None)
    assert lib.adrp_dslpid_compute(None, 1 / 48, None, None, None, 0, 0, None, None, None, None, None, None, None, None) == abi.ERR_INVALID
    assert b"NULL argument" in lib.adrp_last_error(None)
    assert lib.adrp_dslpid_reset(None, None, None) == abi.ERR_INVALID
    assert lib.adrp_dslpid_set_gains(None, ctypes.byref(p)) == abi.ERR_INVALID


def test_python_class_refusals():
    from gym_pybullet_adrp_amd.control import DSLPIDControl
    from gym_pybullet_adrp_amd.control.DSLPIDControl import DSLPIDControl as Direct
    from gym_pybullet_adrp_amd.control.DSLPIDControl import check_input_shape, check_target_shape
    assert DSLPIDControl is Direct
    with pytest.raises(ValueError, match="requires DroneModel.CF2X or DroneModel.CF2P"):
        DSLPIDControl(DroneModel.RACE)
    with pytest.raises(ValueError, match="precision"):
        DSLPIDControl(DroneModel.CF2X, precision="fp16")
    for ok in ((3,), (5, 3), (7, 5, 3)):
        check_target_shape("target_pos", ok, 7, 5)
    for bad in ((4,), (7, 3), (5, 7, 3), (7, 5, 4), (1, 3), ()):
        with pytest.raises(ValueError, match="target_pos must have shape"):
            check_target_shape("target_pos", bad, 7, 5)
    check_input_shape("cur_quat", (7, 5, 4), 7, 5, 4)
    for bad in ((7, 5, 3), (35, 4), (5, 7, 4), (4,)):
        with pytest.raises(ValueError, match="cur_quat must have shape"):
            check_input_shape("cur_quat", bad, 7, 5, 4)


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from gym_pybullet_adrp_amd import _lib
    from gym_pybullet_adrp_amd.control import DSLPIDControl
    with pytest.raises(_lib.AdrpError):
        DSLPIDControl(DroneModel.CF2P, num_envs=4, num_drones=2)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_formation_is_the_fixtures(fx, N):
    """utils/formations.circle, which tools/pid.py flies, gives the start poses, counters and targets the fixture's
    reference loop was run with"""
    from gym_pybullet_adrp_amd.utils.formations import advance, circle, downwash
    xyzs, rpys, table, wp = circle(N, 48, 1.0)
    case = f"loop_x{N}"
    np.testing.assert_array_equal(xyzs, fx[f"{case}_init_xyzs"])
    np.testing.assert_array_equal(rpys, fx[f"{case}_trpy"])
    assert table.shape == (480, 2)
    for t in range(fx[f"{case}_wp"].shape[0]):
        np.testing.assert_array_equal(wp, fx[f"{case}_wp"][t])
        np.testing.assert_array_equal(np.column_stack([table[wp], xyzs[:, 2]]), fx[f"{case}_tpos"][t])
        wp = advance(wp, table)
    assert advance(np.array([479]), table)[0] == 0
    x2, r2, t2, w2 = downwash(48)
    assert x2.shape == (2, 3) and not r2.any() and t2.shape == (240, 2) and list(w2) == [0, 120] and t2[0, 0] == -t2[120, 0] == 0.5
