"""Stand-alone batched DSLPIDControl (csrc/dslpid_kernel.h, gym_pybullet_adrp_amd/control).  Needs an MI355X: -m gpu.

References: the reference's own computeControl sequences (tests/golden/pid_golden.npz dsl_*, dslpid_golden.npz) and
its examples/pid.py loop on CtrlAviary (dslpid_golden.npz loop_*), the numpy restatement pinned to them
(tests/dslpid_reference.py, tests/test_dslpid.py), and the fused controller of VelocityAviary.

Bar (tests/test_hover_gpu.py, test_multihover_gpu.py): per vector |x - x_ref| <= rtol * max(|x_ref|, floor), rtol
1e-9 (fp64) / 1e-4 (fp32); floors 1.0 for RPMs (``last_rpm``), 1e-3 for pos_e, yaw_e and the controller state
vectors (PID_GROUPS), FLOORS for env state.

Shapes: rows = 1, 48 (a partial wave) and 130 = 26 x 5 (two waves and two lanes).  No test asserts flight quality
(DESIGN.md §6).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ctrl_cases as cc  # noqa: E402
import dslpid_reference as ref  # noqa: E402
from gym_pybullet_adrp_amd.control import DSLPIDControl  # noqa: E402
from gym_pybullet_adrp_amd.envs import CtrlAviary, VelocityAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import DroneModel, Physics  # noqa: E402
from test_ctrl_gpu import assert_groups, assert_rows, random_state  # noqa: E402
from test_hover_gpu import FLOORS, GROUPS, PID_GROUPS  # noqa: E402
from test_multihover_gpu import F32_ULP, RTOL, field_index, get_state, put_state, real_of  # noqa: E402

MODEL = {"x": DroneModel.CF2X, "p": DroneModel.CF2P}
NP_REAL = {"fp64": np.float64, "fp32": np.float32}
assert FLOORS["last_rpm"] == 1.0 and all(FLOORS[g] == 1e-3 for g in PID_GROUPS) and tuple(PID_GROUPS) == ref.STATE_GROUPS


@pytest.fixture(scope="module")
def fx():
    return ref.load()


def dev(a, precision):
    return torch.from_numpy(np.ascontiguousarray(a).astype(NP_REAL[precision])).cuda()


def host(t):
    return t.double().cpu().numpy()


def check(ctrl, outs, want, rtol, what):
    """outputs [E, N, .] and the controller's state against (rpm, pos_e, yaw_e, state [K, 9]) of a reference"""
    K = ctrl.rows
    rpm, pos_e, yaw_e = (host(o).reshape(K, -1) for o in outs)
    st = host(ctrl.get_state()).T
    ref.assert_outputs(rpm, pos_e, yaw_e[:, 0], st, want[0], want[1], want[2], want[3], rtol, what)


# ---------------------------------------------------------------------------------------------
# 1  the existing reference sequences (pid_golden.npz dsl_*, CF2X, dt = 1/30)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_existing_reference_sequences(precision):
    import os
    pg = np.load(os.path.join(cc.ROOT, "tests", "golden", "pid_golden.npz"))
    cin, want_rpm, want_st = pg["dsl_in"], pg["dsl_rpm"], pg["dsl_state"]
    S, T = cin.shape[:2]
    assert (S, T) == (48, 12)
    rtol = RTOL[precision]
    a = DSLPIDControl(DroneModel.CF2X, num_envs=S, num_drones=1, precision=precision)
    b = DSLPIDControl(DroneModel.CF2X, num_envs=26, num_drones=5, precision=precision)
    tile = np.arange(130) % S
    rng = np.random.default_rng(5)
    for t in range(T):
        i = cin[:, t]
        outs = a.computeControl(1 / 30, dev(i[:, None, 0:3], precision), dev(i[:, None, 3:7], precision),
                                dev(i[:, None, 7:10], precision), None, dev(i[:, None, 10:13], precision),
                                dev(i[:, None, 13:16], precision), dev(i[:, None, 16:19], precision))
        st = host(a.get_state()).T
        assert ref.vec_err(host(outs[0]).reshape(S, 4), want_rpm[:, t], 1.0).max() <= rtol, f"t={t} rpm"
        for k, g in enumerate(ref.STATE_GROUPS):
            assert ref.vec_err(st[:, 3 * k:3 * k + 3], want_st[:, t, 3 * k:3 * k + 3], 1e-3).max() <= rtol, f"t={t} {g}"
        # tiled to 130 rows through state rows; the columns the controller does not read hold NaN
        rows = np.full((130, 20), np.nan)
        rows[:, 0:3], rows[:, 3:7], rows[:, 10:13] = i[tile, 0:3], i[tile, 3:7], i[tile, 7:10]
        rows[:, 13:16] = rng.normal(size=(130, 3))       # cur_ang_vel: unused by the reference
        rpm_b, pos_e_b, yaw_e_b = b.computeControlFromState(1 / 30, dev(rows.reshape(26, 5, 20), precision),
                                                            dev(i[tile, 10:13].reshape(26, 5, 3), precision),
                                                            dev(i[tile, 13:16].reshape(26, 5, 3), precision),
                                                            dev(i[tile, 16:19].reshape(26, 5, 3), precision))
        stb = b.get_state()
        assert ref.vec_err(host(rpm_b).reshape(130, 4), want_rpm[tile, t], 1.0).max() <= rtol, f"t={t} tiled rpm"
        for k, g in enumerate(ref.STATE_GROUPS):
            assert ref.vec_err(host(stb).T[:, 3 * k:3 * k + 3], want_st[tile, t, 3 * k:3 * k + 3], 1e-3).max() <= rtol, f"t={t} tiled {g}"
        for lo in (48, 96):
            n = min(48, 130 - lo)
            assert torch.equal(rpm_b.reshape(130, 4)[lo:lo + n], rpm_b.reshape(130, 4)[:n]), f"t={t} copies differ"
            assert torch.equal(pos_e_b.reshape(130, 3)[lo:lo + n], pos_e_b.reshape(130, 3)[:n])
            assert torch.equal(yaw_e_b.reshape(130)[lo:lo + n], yaw_e_b.reshape(130)[:n])
            assert torch.equal(stb[:, lo:lo + n], stb[:, :n])
        assert torch.equal(rpm_b.reshape(130, 4)[:48], outs[0].reshape(48, 4))       # and equal to the 48-row run
    assert a.control_counter == T == b.control_counter
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------
# 2  the new sequences: both mixers, rates, yaw targets, pos_e, yaw_e, the gain group
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("tag", ["x", "p"])
def test_new_sequences(fx, tag, precision):
    rtol = RTOL[precision]
    cin, flags = fx[f"{tag}_in"], fx[f"{tag}_flags"]
    T = cin.shape[1]
    assert all(flags[..., k].any() for k in range(7)) and (flags[..., 5] & 1).any() and (flags[..., 5] & 2).any()
    assert (cin[..., 19:22] != 0).any() and (cin[..., 15] != 0).any() and (flags[..., 4] == 0).any()
    for name, sel in (("default", slice(0, 16)), ("gains", slice(16, 24))):
        S = cin[sel].shape[0]
        c = DSLPIDControl(MODEL[tag], num_envs=S, num_drones=1, precision=precision)
        assert c.GRAVITY == float(fx[f"{tag}_GRAVITY"]) and c.KF == float(fx[f"{tag}_KF"]) and c.KM == float(fx[f"{tag}_KM"])
        np.testing.assert_array_equal(c.MIXER_MATRIX, fx[f"{tag}_MIXER"])
        if name == "gains":
            c.setPIDCoefficients(**ref.fixture_gains(fx, keyword=True))
            np.testing.assert_array_equal(c.P_COEFF_TOR, fx["gains_p_coeff_att"])
            assert flags[sel].any()
        c.set_state(torch.from_numpy(fx[f"{tag}_st0"][sel].T.copy()))
        for t in range(T):
            i = cin[sel, t]
            outs = c.computeControl(float(fx["dt"]), *(dev(i[:, None, s], precision) for s in (slice(0, 3), slice(3, 7), slice(7, 10))),
                                    None, *(dev(i[:, None, s], precision) for s in (slice(10, 13), slice(13, 16), slice(16, 19), slice(19, 22))))
            check(c, outs, (fx[f"{tag}_rpm"][sel, t], fx[f"{tag}_pos_e"][sel, t], fx[f"{tag}_yaw_e"][sel, t], fx[f"{tag}_state"][sel, t]),
                  rtol, f"{tag} {name} t={t} ")
        c.close()


# ---------------------------------------------------------------------------------------------
# 3  the examples/pid.py loop on CtrlAviary, teacher-forced per step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("tag", ["x", "p"])
def test_pid_loop_replay(fx, tag, N, precision):
    """Per step: the fixture's rows into a CtrlAviary and the controllers' state into the controller,
    computeControlFromState(env) against what the reference's controllers returned and held, then env.step(rpm)
    (float64: unrounded) against the rows after.

    Measured on the MI355X, worst figure of the six cases in the bar's measure, fp64 / fp32: RPMs 5.4e-15 / 2.1e-6,
    pos_e 0 / 2.7e-5, yaw_e 4.4e-13 / 4.7e-5, last_rpy 1.0e-13 / 2.1e-7, integral_pos_e 1.6e-16 / 2.0e-6,
    integral_rpy_e 2.4e-14 / 2.6e-6.  The float32 yaw error is what rounding the fixture's float64 state to float32
    leaves (the float64 restatement on the rounded inputs gives the same 4.7e-5): the float32 kernel evaluates it in
    float64 from its float32 operands (csrc/dslpid_kernel.h yaw_error)."""
    rtol = RTOL[precision]
    case = f"loop_{tag}{N}"
    T = fx[f"{case}_obs"].shape[0]
    env = CtrlAviary(num_drones=N, initial_xyzs=fx[f"{case}_init_xyzs"], initial_rpys=fx[f"{case}_trpy"], physics=Physics.DYN,
                     pyb_freq=240, ctrl_freq=48, num_envs=1, precision=precision)
    ctrl = DSLPIDControl(MODEL[tag], num_envs=1, num_drones=N, precision=precision)
    idx, iidx, names = field_index(env)
    groups = {"pos", "quat", "vel", "omega", "angv", "last_rpm"}
    tpos, trpy = dev(fx[f"{case}_tpos"][:, None], precision), dev(fx[f"{case}_trpy"][None], precision)

    def step_from(rows_before, action, t):
        """env.step(action) from the fixture's rows before step t, against its rows after"""
        i = np.zeros((3, N), np.int32)
        i[iidx["step_counter"]] = 5 * t
        put_state(env, cc.fill_state(names, rows_before), i)
        obs, _, _, _, _ = env.step(action)
        torch.cuda.synchronize()
        want = ref.loop_rows_after(fx, case, t)
        assert_rows(obs.cpu().numpy().reshape(N, 20), want, rtol + F32_ULP, f"{case} t={t} ")
        fg, _ = get_state(env)
        assert_groups(fg, cc.fill_state(names, want), idx, groups, rtol, f"{case} t={t} ")

    step_from(ref.loop_rows_before(fx, case, 0), torch.zeros((1, N, 4), dtype=ctrl.real, device=env.device), 0)
    for t in range(T):
        i = np.zeros((3, N), np.int32)
        i[iidx["step_counter"]] = 5 * (t + 1)
        put_state(env, cc.fill_state(names, ref.loop_rows_after(fx, case, t)), i)
        ctrl.set_state(torch.from_numpy(ref.loop_ctl_before(fx, case, t).T.copy()))
        rpm, pos_e, yaw_e = ctrl.computeControlFromState(env.CTRL_TIMESTEP, env, tpos[t], trpy)
        check(ctrl, (rpm, pos_e, yaw_e), (fx[f"{case}_rpm"][t], fx[f"{case}_pos_e"][t], fx[f"{case}_yaw_e"][t], fx[f"{case}_ctl"][t]),
              rtol, f"{case} t={t} ")
        if t + 1 < T:
            assert rpm.dtype == (torch.float64 if precision == "fp64" else torch.float32)      # handed over unrounded
            step_from(ref.loop_rows_after(fx, case, t), rpm, t + 1)
    env.close(); ctrl.close()


# ---------------------------------------------------------------------------------------------
# 4  the three input layouts agree bit for bit
# ---------------------------------------------------------------------------------------------
def rows_of(env):
    """[E, N, 20] rows in the env's precision from its state columns (pos, quat, vel; NaN elsewhere)"""
    idx, _, _ = field_index(env)
    f, _ = env.get_state()
    E, N = env.num_envs, env.NUM_DRONES
    rows = torch.full((E * N, 20), float("nan"), dtype=f.dtype, device=f.device)
    for k, ax in enumerate("xyz"):
        rows[:, k] = f[idx[f"pos_{ax}"]]; rows[:, 10 + k] = f[idx[f"vel_{ax}"]]
    for k, ax in enumerate("xyzw"):
        rows[:, 3 + k] = f[idx[f"quat_{ax}"]]
    return rows.reshape(E, N, 20).contiguous()


def random_ctl(rng, K):
    st = np.zeros((9, K))
    st[0:3] = rng.uniform(-0.2, 0.2, (3, K))
    st[3:6] = rng.uniform(-1, 1, (3, K)) * np.array([[2], [2], [0.15]])
    st[6:9] = rng.uniform(-1, 1, (3, K)) * np.array([[1], [1], [20]])
    return st


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_layouts_agree(precision):
    E, N = 26, 5
    rng = np.random.default_rng(40)
    env = CtrlAviary(num_drones=N, physics=Physics.PYB, pyb_freq=240, ctrl_freq=48, num_envs=E, precision=precision)
    f, i = random_state(rng, env)
    put_state(env, f, i)
    st0 = torch.from_numpy(random_ctl(rng, E * N))
    tgt = [dev(rng.uniform(-1, 1, (E, N, 3)), precision) for _ in range(4)]
    rows = rows_of(env)
    results = []
    for layout in ("handle", "rows", "arrays"):
        c = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision=precision)
        c.set_state(st0)
        if layout == "handle":
            outs = c.computeControlFromState(1 / 48, env, *tgt)
        elif layout == "rows":
            outs = c.computeControlFromState(1 / 48, rows, *tgt)
        else:
            outs = c.computeControl(1 / 48, rows[..., 0:3].contiguous(), rows[..., 3:7].contiguous(), rows[..., 10:13].contiguous(),
                                    None, *tgt)
        results.append([o.clone() for o in outs] + [c.get_state()])
        c.close()
    for other, name in ((results[1], "rows"), (results[2], "arrays")):
        for a, b, what in zip(results[0], other, ("rpm", "pos_e", "yaw_e", "state")):
            assert torch.equal(a, b), f"{name} {what} differs from the handle path"
    assert torch.isfinite(results[0][0]).all()
    if precision == "fp64":   # float32 rows into the float64 controller: the float64 rows rounded to float32 first
        outs = []
        for r in (rows.float(), rows.float().double()):
            c = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision="fp64")
            c.set_state(st0)
            o = c.computeControlFromState(1 / 48, r, *tgt)
            outs.append([x.clone() for x in o] + [c.get_state()])
            c.close()
        assert outs[0][0].dtype == torch.float64
        for a, b, what in zip(outs[0], outs[1], ("rpm", "pos_e", "yaw_e", "state")):
            assert torch.equal(a, b), f"float32 rows: {what}"
        assert not torch.equal(outs[0][0], results[0][0])          # (and the rounding is visible)
    else:
        c = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision="fp32")
        with pytest.raises(ValueError, match="float32 into a float64"):
            c.computeControlFromState(1 / 48, rows.double(), *tgt)
        env64 = CtrlAviary(num_drones=N, num_envs=E, precision="fp64")
        with pytest.raises(ValueError, match="the controller"):
            c.computeControlFromState(1 / 48, env64, *tgt)
        env64.close(); c.close()
    env.close()


# ---------------------------------------------------------------------------------------------
# 5  the stand-alone controller against the controller fused into VelocityAviary's step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("physics", [Physics.DYN, Physics.PYB])
def test_standalone_matches_fused(physics, precision):
    E, N, rtol = 40, 3, RTOL[precision]
    K = E * N
    rng = np.random.default_rng(500 + (physics == Physics.PYB))
    env = VelocityAviary(num_drones=N, physics=physics, pyb_freq=240, ctrl_freq=48, num_envs=E, precision=precision)
    idx, iidx, names = field_index(env)
    f, i = random_state(rng, env, tilt=0.15, omega=1.0, pid=True)
    put_state(env, f, i)
    a = rng.uniform(-1, 1, (E, N, 4)).astype(np.float32)
    a[..., :3] = np.round(a[..., :3] * 64) / 64          # exact float32 sum of squares in any order
    a[..., 3] = np.abs(a[..., 3])
    a[::7, 0, :3] = 0
    env.step(torch.from_numpy(a))
    fg, _ = get_state(env)
    # the same controller call, stand-alone, from the pre-step state
    cols = lambda g: f[[idx[n] for n in GROUPS[g]]].T        # noqa: E731
    pos, quat, vel = cols("pos"), cols("quat"), cols("vel")
    yaw = ref.euler_xyz(quat)[:, 2]                          # host float64, from the quaternion
    af = a.reshape(K, 4)
    n = np.sqrt((af[:, 0] * af[:, 0] + af[:, 1] * af[:, 1] + af[:, 2] * af[:, 2]).astype(np.float64)).astype(np.float32)
    s = np.float32(env.SPEED_LIMIT) * np.abs(af[:, 3])
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (af[:, :3].astype(np.float64) / n.astype(np.float64)[:, None]).astype(np.float32)
    tv = np.where(n[:, None] != 0, s[:, None] * d, np.float32(0)).astype(np.float32)
    assert tv.dtype == np.float32 and (n == 0).any()
    ctrl = DSLPIDControl(DroneModel.CF2X, num_envs=E, num_drones=N, precision=precision)
    ctrl.set_state(torch.from_numpy(np.stack([f[idx[nme]] for nme in cc.PID_NAMES])))
    trpy = np.zeros((K, 3)); trpy[:, 2] = yaw
    sh = lambda x: dev(x.reshape(E, N, -1), precision)       # noqa: E731
    rpm, _, _ = ctrl.computeControl(env.CTRL_TIMESTEP, sh(pos), sh(quat), sh(vel), None, sh(pos), sh(trpy), sh(tv.astype(np.float64)))
    got_rpm = host(rpm).reshape(K, 4)
    want_rpm = fg[[idx[n] for n in GROUPS["last_rpm"]]].T
    assert ref.vec_err(got_rpm, want_rpm, FLOORS["last_rpm"]).max() <= rtol
    st = host(ctrl.get_state())
    for g in PID_GROUPS:
        rows = [cc.PID_NAMES.index(n) for n in PID_GROUPS[g]]
        err = cc.vec_err(st[rows].T, fg[[idx[n] for n in PID_GROUPS[g]]].T, FLOORS[g])
        assert err.max() <= rtol, f"{g}: {err.max():.3e}"
    env.close(); ctrl.close()


# ---------------------------------------------------------------------------------------------
# 6  batch invariance, masked reset, the call counter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_batch_invariance_and_masks(precision):
    E, N = 26, 5
    K = E * N
    rng = np.random.default_rng(60)
    pos, vel = rng.uniform(-1, 1, (E, N, 3)), rng.uniform(-1, 1, (E, N, 3))
    quat = rng.normal(size=(E, N, 4)); quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    quat[..., 3] = np.abs(quat[..., 3]) + 2.0; quat /= np.linalg.norm(quat, axis=-1, keepdims=True)    # moderate tilts
    tgt = [rng.uniform(-1, 1, (E, N, 3)) for _ in range(4)]
    st0 = random_ctl(rng, K)
    big = DSLPIDControl(DroneModel.CF2X, num_envs=E, num_drones=N, precision=precision)
    big.set_state(torch.from_numpy(st0))
    assert big.control_counter == 0
    outs = big.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None,
                              *(dev(t, precision) for t in tgt))
    assert big.control_counter == 1
    st = big.get_state()
    for r in (0, 77, 129):
        e, n = divmod(r, N)
        one = DSLPIDControl(DroneModel.CF2X, num_envs=1, num_drones=1, precision=precision)
        one.set_state(torch.from_numpy(st0[:, r:r + 1].copy()))
        o = one.computeControl(1 / 48, dev(pos[e:e + 1, n:n + 1], precision), dev(quat[e:e + 1, n:n + 1], precision),
                               dev(vel[e:e + 1, n:n + 1], precision), None, *(dev(t[e:e + 1, n:n + 1], precision) for t in tgt))
        assert torch.equal(o[0][0, 0], outs[0][e, n]) and torch.equal(o[1][0, 0], outs[1][e, n]) and torch.equal(o[2][0, 0], outs[2][e, n])
        assert torch.equal(one.get_state()[:, 0], st[:, r]), f"row {r}"
        one.close()
    assert (st != 0).all(dim=0).any()
    # reset(mask): exactly the masked controllers
    mask = rng.random((E, N)) < 0.4
    assert mask.any() and not mask.all()
    big.reset(mask)
    assert big.control_counter == 0
    st1 = big.get_state()
    m = torch.from_numpy(mask.reshape(K)).cuda()
    assert (st1[:, m] == 0).all() and torch.equal(st1[:, ~m], st[:, ~m])
    big.set_state(st)
    emask = np.arange(E) % 3 == 0                         # per env: all of its drones
    big.reset(emask)
    st2 = big.get_state()
    m = torch.from_numpy(np.repeat(emask, N)).cuda()
    assert (st2[:, m] == 0).all() and torch.equal(st2[:, ~m], st[:, ~m])
    big.reset()
    assert (big.get_state() == 0).all()
    for k in range(3):
        big.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None, dev(tgt[0], precision))
    assert big.control_counter == 3
    # broadcast targets: [3] and [N, 3] are the expanded [E, N, 3]
    a = [x.clone() for x in big.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None,
                                               tgt[0][0, 0], tgt[1][0])]
    big.reset()
    for k in range(3):
        big.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None, dev(tgt[0], precision))
    b = big.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None,
                           dev(np.broadcast_to(tgt[0][0, 0], (E, N, 3)), precision), dev(np.broadcast_to(tgt[1][0], (E, N, 3)), precision))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="target_pos must have shape"):
        big.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None, np.zeros((E, 3)))
    with pytest.raises(ValueError, match="cur_quat must have shape"):
        big.computeControl(1 / 48, dev(pos, precision), dev(quat[..., :3], precision), dev(vel, precision), None, np.zeros(3))
    with pytest.raises(ValueError, match="control_timestep must be > 0"):
        big.computeControl(0.0, dev(pos, precision), dev(quat, precision), dev(vel, precision), None, np.zeros(3))
    big.close()


# ---------------------------------------------------------------------------------------------
# 7  step + computeControlFromState(env) captured in one HIP graph replays the eager bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_graph_replay_is_eager(precision):
    E, N, ITERS = 26, 5, 8
    rng = np.random.default_rng(70)
    env = CtrlAviary(num_drones=N, physics=Physics.PYB, pyb_freq=240, ctrl_freq=48, num_envs=E, precision=precision)
    ctrl = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision=precision)
    f, i = random_state(rng, env, tilt=0.1, vel=0.2, omega=0.5)
    cols = lambda g: f[[field_index(env)[0][n] for n in GROUPS[g]]].T        # noqa: E731
    tpos = dev((cols("pos") + rng.uniform(-0.1, 0.1, (E * N, 3))).reshape(E, N, 3), precision)
    rpm0 = dev(np.full((E, N, 4), env.HOVER_RPM), precision)
    st0 = torch.from_numpy(random_ctl(rng, E * N))
    rpm, pos_e, yaw_e = (torch.zeros(s, dtype=ctrl.real, device=env.device) for s in ((E, N, 4), (E, N, 3), (E, N)))

    def start():
        put_state(env, f, i)
        ctrl.set_state(st0)
        rpm.copy_(rpm0)

    def loop():
        for _ in range(ITERS):
            env.step(rpm)
            ctrl.computeControlFromState(env.CTRL_TIMESTEP, env, tpos, out=(rpm, pos_e, yaw_e))

    def snapshot():
        torch.cuda.synchronize()
        return [x.clone() for x in (env._obs, *env.get_state(), ctrl.get_state(), rpm, pos_e, yaw_e)]

    start(); loop()
    eager = snapshot()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        start(); loop()                                   # warm the side stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            loop()
    start()
    torch.cuda.synchronize()
    g.replay()
    replayed = snapshot()
    assert ctrl.control_counter == 3 * ITERS               # (the capture counted its calls; replays are the device's)
    for a, b, what in zip(eager, replayed, ("obs", "state", "ints", "controller state", "rpm", "pos_e", "yaw_e")):
        assert torch.equal(a, b), what
    assert torch.isfinite(eager[0]).all() and not torch.equal(eager[4], rpm0)
    env.close(); ctrl.close()


# ---------------------------------------------------------------------------------------------
# 8  the other envs' handles: hover tasks are read like CtrlAviary's, a race handle is refused
# ---------------------------------------------------------------------------------------------
def test_other_env_handles():
    from gym_pybullet_adrp_amd.envs import HoverAviary, MultiHoverAviary, MultiRaceAviary
    rng = np.random.default_rng(80)
    for env in (HoverAviary(num_envs=48, precision="fp64", autoreset=False, seed=3, init_noise={"xyz": 0.2, "rpy": 0.2, "vel": 0.3}),
                MultiHoverAviary(num_drones=5, num_envs=9, precision="fp32", autoreset=False, seed=4,
                                 init_noise={"xyz": 0.1, "rpy": 0.2, "vel": 0.3})):
        env.reset()
        E, N = env.num_envs, getattr(env, "NUM_DRONES", 1)
        precision = "fp64" if env.h.real == torch.float64 else "fp32"
        tgt = dev(rng.uniform(-1, 1, (E, N, 3)), precision)
        outs = []
        for state in (env, rows_of(env)):
            c = DSLPIDControl(DroneModel.CF2X, num_envs=E, num_drones=N, precision=precision)
            outs.append([x.clone() for x in c.computeControlFromState(1 / 48, state, tgt)] + [c.get_state()])
            c.close()
        assert all(torch.equal(a, b) for a, b in zip(*outs)) and torch.isfinite(outs[0][0]).all()
        assert not torch.equal(outs[0][1][0, 0], outs[0][1][-1, -1])      # (pos_e: the rows hold different states)
        env.close()
    race = MultiRaceAviary("level0", num_drones=2, num_envs=4, seed=3, autoreset=False)
    race.reset()
    c = DSLPIDControl(DroneModel.CF2X, num_envs=4, num_drones=2, precision="fp64" if race.h.real == torch.float64 else "fp32")
    with pytest.raises(ValueError, match="MultiRaceAviary handles are not supported"):
        c.computeControlFromState(1 / 48, race, np.zeros(3))
    race.close(); c.close()


# ---------------------------------------------------------------------------------------------
# 9  the C entry point's own refusals of an env handle (the Python class checks the same before it calls)
# ---------------------------------------------------------------------------------------------
def test_compute_env_refusals_in_c():
    import ctypes
    from gym_pybullet_adrp_amd import _lib
    from gym_pybullet_adrp_amd.envs import HoverAviary
    from gym_pybullet_adrp_amd.utils import abi
    lib = _lib.load()
    ctrl = DSLPIDControl(DroneModel.CF2X, num_envs=6, num_drones=2, precision="fp64")
    rpm = torch.zeros((6, 2, 4), dtype=torch.float64, device="cuda")

    def refused(env, msg):
        rc = lib.adrp_dslpid_compute_env(ctrl.h, 1 / 48, env.h.h, None, None, None, None, _lib._p(rpm), None, None, None)
        assert rc == abi.ERR_INVALID and msg in lib.adrp_last_error(None), lib.adrp_last_error(None)

    small = CtrlAviary(num_drones=2, num_envs=5, precision="fp64")
    refused(small, b"E * N differs from the controller's rows")
    single = CtrlAviary(num_drones=2, num_envs=6, precision="fp32")
    refused(single, b"precision differs from the controller's")
    hover = HoverAviary(num_envs=12, precision="fp64", autoreset=False)
    hover.reset()
    with hover.persistent():
        refused(hover, b"persistent mode is active")
    good = CtrlAviary(num_drones=2, num_envs=6, precision="fp64")
    good.reset()
    assert lib.adrp_dslpid_compute_env(ctrl.h, 1 / 48, good.h.h, None, None, None, None, _lib._p(rpm), None, None, None) == 0
    assert lib.adrp_dslpid_compute_env(ctrl.h, 1 / 48, None, None, None, None, None, _lib._p(rpm), None, None, None) == abi.ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isfinite(rpm).all() and (rpm > 0).all()
    for e in (small, single, hover, good):
        e.close()
    ctrl.close()


# ---------------------------------------------------------------------------------------------
# 10  numpy inputs are copied in the controller's dtype; outputs the caller does not bind are not written
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_numpy_inputs_and_optional_outputs(precision):
    E, N = 7, 3
    rng = np.random.default_rng(90)
    pos, vel, tgt = rng.uniform(-1, 1, (E, N, 3)), rng.uniform(-1, 1, (E, N, 3)), rng.uniform(-1, 1, (E, N, 3))
    quat = rng.normal(size=(E, N, 4)); quat[..., 3] = np.abs(quat[..., 3]) + 2.0
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    a = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision=precision)
    b = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision=precision)
    assert pos.dtype == np.float64
    from_numpy = [x.clone() for x in a.computeControl(1 / 48, pos, quat, vel, None, tgt)]     # float64 numpy, either controller
    from_tensor = b.computeControl(1 / 48, dev(pos, precision), dev(quat, precision), dev(vel, precision), None, dev(tgt, precision))
    assert all(torch.equal(x, y) for x, y in zip(from_numpy, from_tensor)) and torch.equal(a.get_state(), b.get_state())
    rows = np.zeros((E, N, 20)); rows[..., 0:3], rows[..., 3:7], rows[..., 10:13] = pos, quat, vel
    a.reset(); b.reset()
    rpm = torch.zeros((E, N, 4), dtype=a.real, device="cuda")
    keep = torch.full((E, N), 7.0, dtype=a.real, device="cuda")
    out = a.computeControlFromState(1 / 48, rows.tolist(), tgt, out=(rpm, None, None))
    assert out[0] is rpm and out[1] is None and out[2] is None and torch.equal(rpm, from_numpy[0])
    b.computeControlFromState(1 / 48, rows, tgt, out=(rpm, None, keep))     # (a bound tensor is written)
    assert torch.equal(keep, from_numpy[2])
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------
# 11  DeviceLogger on CtrlAviary: the RPM columns are the applied RPMs in a physics mode without drag
# ---------------------------------------------------------------------------------------------
def test_device_logger_logs_applied_rpms():
    from gym_pybullet_adrp_amd.logger import DeviceLogger
    E, N = 3, 2
    rng = np.random.default_rng(110)
    env = CtrlAviary(num_drones=N, physics=Physics.PYB, pyb_freq=240, ctrl_freq=48, num_envs=E, precision="fp64")
    env.reset()
    logger = DeviceLogger(env, logging_freq_hz=48, slots=[0, 1, 5], duration_steps=2)
    rpm = torch.from_numpy(env.HOVER_RPM * rng.uniform(0.9, 1.1, (E, N, 4))).cuda()
    obs, _, _, _, _ = env.step(rpm)
    logger.log(0.0)
    st = logger.states[0]
    assert torch.equal(st[:, 16:20], rpm.reshape(E * N, 4)[[0, 1, 5]])
    assert torch.equal(st[:, 0:3].float(), obs.reshape(E * N, 20)[[0, 1, 5], 0:3])
    ts, states, controls = logger.arrays()
    assert states.shape == (3, 16, 1) and np.array_equal(states[:, 12:16, 0], rpm.reshape(E * N, 4)[[0, 1, 5]].cpu().numpy())
    env.close()
