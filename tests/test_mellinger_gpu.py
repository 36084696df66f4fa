"""Stand-alone MellingerControl (csrc/mellinger_kernel.h) against the CPU oracle, one controller call at a time.
Needs an MI355X: -m gpu.

The yardstick is the unchanged oracle as a race env at pyb_freq = ctrl_freq = 500 without auto-reset: one
Oracle.step is one physics sub-step followed by one mellinger_compute call per drone (oracle/race.c
race_step_env).  A per-call comparison copies the oracle's controller and command state into the stand-alone
handle by field name, steps the oracle, calls compute once with the oracle's post-step position, roll / pitch / yaw
(O.euler_from_quat of its quaternion) and velocity and the injected thrust noise, and reads the handle's state.

Bars (tests/test_race_gpu.py's): the ints are equal; the int16 moments within one count of the oracle's own;
with the oracle re-run from the same state on the kernel's moments (set_moment_replay), every float field within
FP64_BAR = 1e-6 relative in fp64 and RTOL["fp32"] = 2e-3 in fp32 (floors: rpm 1.0, the rest 1e-3); the share of
calls whose own truncation differed at most DIFFER_MAX.  Measured shares and errors: DESIGN.md §3.16.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.commands import encode_commands  # noqa: E402
from gym_pybullet_adrp_amd.control import MellingerControl  # noqa: E402
from gym_pybullet_adrp_amd.control.MellingerControl import pack_command  # noqa: E402
from gym_pybullet_adrp_amd.envs import CtrlAviary, HoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Command, DroneModel, Physics, RaceMode  # noqa: E402
from oracle import oracle as O  # noqa: E402

from test_commander_gpu import CMD_GROUPS, CMD_TOL, COEF, DUR, T0  # noqa: E402
from test_race_gpu import DIFFER_MAX, FP64_BAR, RTOL  # noqa: E402

SHAPES = [(1, 1), (3, 2), (32, 2), (9, 8)]
BAR = {"fp64": FP64_BAR, "fp32": RTOL["fp32"]}
RPM_FLOOR = 0.2685 * 20000 + 4070.3          # motors cut: the PWM clip's lower end
MOM_HASH_SEED, MOM_HASH_MUL = 2166136261, 16777619


def make_oracle(E, N, level="level1"):
    """the oracle as a race env whose step is one sub-step and one controller call"""
    env = MultiRaceAviary(level, num_drones=N, physics=Physics.PYB, racemode=RaceMode.COMPARE, num_envs=E, seed=11,
                          autoreset=False, precision="fp64", pyb_freq=500, ctrl_freq=500)
    cfg = env.cfg.copy()
    env.close()
    orc = O.Oracle(cfg)
    assert orc.S == 1
    return orc


class Names:
    def __init__(self, orc, ctl):
        self.of, self.oi = orc.field_names()
        self.cf, self.ci = ctl.state_field_names()
        self.fmap = [self.of.index(n) for n in self.cf]      # oracle row of every controller float field
        self.imap = [self.oi.index(n) for n in self.ci]

    def o(self, name):
        return self.of.index(name)


def f32_representable(f):
    return f.astype(np.float32).astype(np.float64)


def body_of(orc, nm):
    """post-step position, roll / pitch / yaw and velocity [E, N, 3] of the oracle's drones (float64)"""
    f, _ = orc.get_state()
    E, N = orc.E, orc.N
    pos = f[[nm.o("pos_x"), nm.o("pos_y"), nm.o("pos_z")]].T
    vel = f[[nm.o("vel_x"), nm.o("vel_y"), nm.o("vel_z")]].T
    quat = f[[nm.o("quat_x"), nm.o("quat_y"), nm.o("quat_z"), nm.o("quat_w")]].T
    rpy = np.stack([O.euler_from_quat(q) for q in quat])
    return pos.reshape(E, N, 3).copy(), rpy.reshape(E, N, 3), vel.reshape(E, N, 3).copy()


def moment_hash(ctl3, ran):
    """fw_moment_hash of one firmware call's int16 moments (race_kernel.h); the seed when no call ran"""
    out = np.full(len(ran), MOM_HASH_SEED, np.uint64)
    for s in np.flatnonzero(ran):
        h = MOM_HASH_SEED
        for v in ctl3[:, s]:
            h = ((h ^ (int(v) & 0xFFFFFFFF)) * MOM_HASH_MUL) & 0xFFFFFFFF
        out[s] = h
    return out.astype(np.uint32)


def field_errors(nm, fg, fo):
    """per controller float field: |gpu - cpu| / max(|cpu|, floor); NaN on both sides (the D term's first call) is
    agreement"""
    want = fo[nm.fmap]
    floor = np.array([1.0 if "rpm" in n else 1e-3 for n in nm.cf])[:, None]
    both_nan = np.isnan(fg) & np.isnan(want)
    err = np.abs(fg - want) / np.maximum(np.abs(want), floor)
    err[both_nan] = 0.0
    assert not np.isnan(err).any(), "NaN on one side only"
    return err


class Stats:
    def __init__(self):
        self.calls = self.differ = 0
        self.worst = self.worst_chain = self.worst_state = 0.0

    def line(self, what):
        share = self.differ / max(self.calls, 1)
        return (f"[mellinger] {what}: {self.calls} calls, {self.differ} with a different own truncation ({share:.2%}), "
                f"max error with the kernel's moments {self.worst:.2e}, PWM chain alone {self.worst_chain:.2e}")

    def check(self):
        share = self.differ / max(self.calls, 1)
        assert share <= DIFFER_MAX, f"{self.differ} of {self.calls} calls truncated differently ({share:.1%} > {DIFFER_MAX:.0%})"


def copy_in(ctl, orc, nm, f, i):
    real = np.float64 if ctl.real == torch.float64 else np.float32
    ctl.set_state(torch.from_numpy(f[nm.fmap].astype(real)), torch.from_numpy(i[nm.imap]))
    ctl.set_command_state(*(torch.from_numpy(a) for a in orc.get_command_state()))


def per_call(ctl, orc, nm, precision, noise, stats, command=None, forced=True, check_cmd_state=True):
    """one controller call on both sides; forced: the handle starts from the oracle's state (else it keeps its
    own).  command: (codes, args) sent to both before the call.  Returns (handle state, oracle state after the
    replay on the kernel's moments), both (float, int)."""
    E, N = orc.E, orc.N
    f0, i0 = orc.get_state()
    if forced:
        f0 = f32_representable(f0)
        orc.set_state(f0, i0)
        copy_in(ctl, orc, nm, f0, i0)
    if command is not None:
        orc.command(*command)
        ctl.command(*command)
    c0 = orc.get_command_state()
    force = np.zeros((E, N, 1, 3))
    orc.set_noise(noise.reshape(E, N, 1, 4), force)
    orc.step(None)
    own_hash = orc.moment_hash()
    fo_own, io_own = orc.get_state()
    assert (io_own[nm.oi.index("flags")] == 0).all(), "a drone was eliminated: the oracle skipped its controller"
    pos, rpy, vel = body_of(orc, nm)
    real = ctl.real
    dev = ctl.device
    rpm = ctl.computeControl(0.002, torch.from_numpy(pos).to(dev, real), torch.from_numpy(rpy).to(dev, real),
                             torch.from_numpy(vel).to(dev, real), disturbance=torch.from_numpy(noise).to(dev, real))
    fg, ig = (t.cpu().numpy() for t in ctl.get_state())
    fg = fg.astype(np.float64)
    rpm = rpm.cpu().numpy().astype(np.float64).reshape(E * N, 4)
    # ---- the ints are equal ----
    for k, n in enumerate(nm.ci):
        np.testing.assert_array_equal(ig[k], io_own[nm.oi.index(n)], err_msg=n)
    # ---- the int16 moments: within one count of the oracle's own truncation ----
    ctl_rows = [nm.cf.index(n) for n in ("ctl_roll", "ctl_pitch", "ctl_yaw")]
    mom_g = fg[ctl_rows]
    mom_o = fo_own[[nm.o(n) for n in ("ctl_roll", "ctl_pitch", "ctl_yaw")]]
    assert (mom_g == np.trunc(mom_g)).all()
    assert np.abs(mom_g - mom_o).max() <= 1.0, f"moments {np.abs(mom_g - mom_o).max()} counts apart"
    tick0 = i0[nm.oi.index("tick")]
    ran = (ig[nm.ci.index("last_att_tick")] == tick0) & (i0[nm.oi.index("last_att_tick")] < tick0)
    cut = ig[nm.ci.index("tumble")] >= 30
    ran &= ~cut
    differ = own_hash != moment_hash(mom_g, ran)
    # ---- replay: the oracle's call from (f0, i0) on the kernel's integers ----
    orc.set_state(f0, i0)
    orc.set_command_state(*c0)
    orc.set_moment_replay(mom_g.T.reshape(E * N, 1, 3).astype(np.int16), np.ones(E * N, np.int32))
    orc.step(None)
    orc.set_moment_replay()
    orc.set_noise()
    np.testing.assert_array_equal(orc.moment_hash(), moment_hash(mom_g, ran))
    fo, io = orc.get_state()
    err = field_errors(nm, fg, fo)
    bar = BAR[precision]
    if not forced:
        # a carried handle's float integrators and filters collect their own float roundings (the kernels' float sin /
        # cos / atan2 are within an ulp of libm's, not equal): the rpm of every tick is what is held to the bar
        stats.worst_state = max(stats.worst_state, float(err.max()))
        err = err[[k for k, n in enumerate(nm.cf) if n.startswith("rpm_")]]
    bad = np.argwhere(err > bar)
    assert len(bad) == 0, (f"{len(bad)} fields over {bar:g} with the kernel's moments: "
                           f"{[(int(a), int(b), float(err[a, b])) for a, b in bad[:6]]} (rows of {'rpm_*' if not forced else 'the state'})")
    np.testing.assert_array_equal(fg[[nm.cf.index(f"rpm_{k}") for k in range(4)]].T, rpm)
    # ---- the PWM chain alone: rpm from the kernel's own controls ----
    ctl4 = fg[[nm.cf.index(n) for n in ("ctl_roll", "ctl_pitch", "ctl_yaw", "ctl_thrust")]].T
    chain = np.stack([O.pwms_to_rpms(np.zeros(4) if cut[s] else O.compute_pwms(ctl4[s]), noise.reshape(-1, 4)[s])
                      for s in range(E * N)])
    cerr = np.abs(rpm - chain) / np.maximum(np.abs(chain), 1.0)
    assert cerr.max() <= bar, f"PWM chain: {cerr.max():.3e} > {bar:g}"
    stats.calls += E * N
    stats.differ += int(differ.sum())
    stats.worst = max(stats.worst, float(err.max()))
    stats.worst_chain = max(stats.worst_chain, float(cerr.max()))
    # ---- command state, field by field ----
    if check_cmd_state:
        check_command_state(ctl, orc, precision)
    return (fg, ig), (fo, io)


def check_command_state(ctl, orc, precision):
    """ints, t_begin and whatever a command copies: exact; evaluated fields: tests/test_commander_gpu.py's bounds
    (setpoints 1e-6, commander position 1e-6, velocity 1e-5, yaw 2e-4 of max(|x|, floor)); the firmware's copy of
    the body state: exact in fp64, one float rounding of the inputs in fp32"""
    fg, ig = (t.cpu().numpy() for t in ctl.get_command_state())
    fo, io = orc.get_command_state()
    np.testing.assert_array_equal(ig, io)
    np.testing.assert_array_equal(fg[T0], fo[T0])
    np.testing.assert_allclose(fg[DUR], fo[DUR], rtol=1e-6)
    np.testing.assert_allclose(fg[COEF:], fo[COEF:], rtol=1e-4, atol=1e-4)
    tol = CMD_TOL["fp64"]
    for g, rows in CMD_GROUPS.items():
        r = list(rows)
        a, b = fg[r].astype(np.float64), fo[r].astype(np.float64)
        if g.startswith("st_"):
            if precision == "fp64":
                np.testing.assert_array_equal(fg[r], fo[r], err_msg=g)
            else:
                np.testing.assert_allclose(a, b, rtol=3e-7, atol=1e-6, err_msg=g)
            continue
        floor = 1.0 if g.endswith("yaw") else 1e-3
        d = np.linalg.norm(a - b, axis=0) / np.maximum(np.linalg.norm(b, axis=0), floor)
        assert d.max() <= tol[g], f"command state {g}: {d.max():.3e} > {tol[g]:.1e}"


def hover_targets(orc, obs0):
    """FULLSTATE 0.5 m above the start, a little to the side per drone"""
    E, N = orc.E, orc.N
    rng = np.random.default_rng(5)
    tgt = obs0[..., :3].astype(np.float64) + rng.uniform(-0.2, 0.2, (E, N, 3)) + [0, 0, 0.5]
    z = np.zeros(3)
    return encode_commands([[(Command.FULLSTATE, [tgt[e, n], z, z, 0.1 * (n - 1), z, 0.0]) for n in range(N)]
                            for e in range(E)], E, N)


def fly(orc, rng, ticks, std):
    """free flight of the oracle under its own controller with injected thrust noise"""
    E, N = orc.E, orc.N
    for _ in range(ticks):
        orc.set_noise(rng.normal(0, std, (E, N, 1, 4)), np.zeros((E, N, 1, 3)))
        orc.step(None)
    orc.set_noise()


def setup(E, N, precision, ticks=100):
    orc = make_oracle(E, N)
    assert orc.cfg.track.disturbances, "level1 has the disturbances on"
    std = orc.cfg.track.action_noise_std
    ctl = MellingerControl(DroneModel.CF2X, num_envs=E, num_drones=N, precision=precision)
    nm = Names(orc, ctl)
    obs0 = orc.reset()
    orc.command(*hover_targets(orc, obs0))
    rng = np.random.default_rng(E * 16 + N)
    fly(orc, rng, ticks, std)
    return orc, ctl, nm, rng, std


# ------------------------------------------------------------------------------------------------------------
# 1. flight states
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("E,N", SHAPES)
def test_flight_states_teacher_forced(E, N, precision):
    orc, ctl, nm, rng, std = setup(E, N, precision)
    stats = Stats()
    for _ in range(40):
        per_call(ctl, orc, nm, precision, rng.normal(0, std, (E, N, 4)), stats)
    print("\n" + stats.line(f"flight states {E}x{N} {precision}"))
    stats.check()
    ctl.close()


# ------------------------------------------------------------------------------------------------------------
# 2. controller state carried, not forced
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("start,ticks", [(0, 300), (990, 120)])
def test_state_carried(start, ticks, precision):
    """the handle gets the oracle's state once and then only the oracle's body states and noise, tick after tick;
    the oracle continues every tick on the kernel's moments (the replay), so both fly the same flight.  From tick
    990 the run crosses tick 1000, after which the float64 schedule skips calls."""
    E, N = 3, 2
    orc, ctl, nm, rng, std = setup(E, N, precision, ticks=0)
    f, i = orc.get_state()
    if start:
        for n, v in (("tick", start), ("last_att_tick", start - 1), ("last_pos_tick", start - 5)):
            i[nm.oi.index(n)] = v
    f = f32_representable(f)
    orc.set_state(f, i)
    copy_in(ctl, orc, nm, f, i)
    stats = Stats()
    skipped = 0
    for k in range(ticks):
        (fg, ig), _ = per_call(ctl, orc, nm, precision, rng.normal(0, std, (E, N, 4)), stats, forced=False)
        np.testing.assert_array_equal(ig[nm.ci.index("tick")], start + k + 1)
        skipped += int((ig[nm.ci.index("last_att_tick")] != start + k).sum())
    print("\n" + stats.line(f"carried from tick {start} {precision}") + f", {skipped} calls without an attitude loop, "
          f"max error of any carried field {stats.worst_state:.2e}")
    stats.check()
    if start:
        assert skipped > 0, "the run did not reach the part of the schedule that skips calls"
    ctl.close()


# ------------------------------------------------------------------------------------------------------------
# 3. constructed ticks
# ------------------------------------------------------------------------------------------------------------
AGES = (0, 1, 5, 6, 999, 1000, 1001, 2500, 4095, 4096, 16000)
DISTANCES = [(da, dp) for da in (1, 2) for dp in (1, 2, 5, 6)]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_constructed_ticks(precision):
    """row (e, n): tick AGES[e], last_att_tick / last_pos_tick at DISTANCES[n] behind it (0 where the tick is
    younger); one call.  Which loops ran is read from last_att_tick / last_pos_tick, equal to the oracle's."""
    E, N = len(AGES), len(DISTANCES)
    orc, ctl, nm, rng, std = setup(E, N, precision)
    f, i = orc.get_state()
    tick = np.repeat(np.array(AGES), N)
    da = np.tile(np.array([d[0] for d in DISTANCES]), E)
    dp = np.tile(np.array([d[1] for d in DISTANCES]), E)
    i[nm.oi.index("tick")] = tick
    i[nm.oi.index("last_att_tick")] = np.maximum(tick - da, 0)
    i[nm.oi.index("last_pos_tick")] = np.maximum(tick - dp, 0)
    orc.set_state(f, i)
    stats = Stats()
    (fg, ig), _ = per_call(ctl, orc, nm, precision, rng.normal(0, std, (E, N, 4)), stats)
    age_a, age_p = tick - np.maximum(tick - da, 0), tick - np.maximum(tick - dp, 0)
    att_ran = (ig[nm.ci.index("last_att_tick")] == tick) & (age_a > 0)
    pos_ran = (ig[nm.ci.index("last_pos_tick")] == tick) & (age_p > 0)
    np.testing.assert_array_equal(ig[nm.ci.index("tick")], tick + 1)
    # two ticks since the attitude loop: always due; none: never.  The position loop runs only with the attitude
    # loop: six ticks since it: always due then; four or fewer: never (race_kernel.h, tick_window)
    assert att_ran[age_a >= 2].all() and not att_ran[age_a == 0].any()
    assert pos_ran[(age_p >= 6) & att_ran].all() and not pos_ran[~att_ran].any() and not pos_ran[age_p <= 4].any()
    assert att_ran[age_a == 1].any() and not att_ran[age_a == 1].all(), "a one-tick age is where float64 rounding decides"
    print("\n" + stats.line(f"constructed ticks {precision}") + f", attitude loop ran in {int(att_ran.sum())} of {E * N}, "
          f"position loop in {int(pos_ran.sum())}")
    ctl.close()


# ------------------------------------------------------------------------------------------------------------
# 4. constructed states
# ------------------------------------------------------------------------------------------------------------
SCENARIOS = ("tumble29", "tumble28", "target_below", "pitch_up", "pitch_down", "yaw_seam", "yaw_seam_crossed",
             "integrators_high", "integrators_low")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_constructed_states(precision):
    E, N = 9, 8
    orc, ctl, nm, rng, std = setup(E, N, precision)
    f, i = orc.get_state()
    rows = np.arange(E * N)
    scen = {s: rows[rows % len(SCENARIOS) == k] for k, s in enumerate(SCENARIOS)}
    noise = rng.normal(0, std, (E * N, 4))
    cf, ci = orc.get_command_state()

    def put(names, cols, values):
        for n, v in zip(names, np.asarray(values, float).T if np.ndim(values) > 1 else values):
            f[nm.o(n), cols] = v

    # tumble counter at 29 / 28 with the vertical velocity falling by 0.2 m/s in the tick: acc_z = -9.2 g
    for s, t in (("tumble29", 29), ("tumble28", 28)):
        i[nm.oi.index("tumble"), scen[s]] = t
        f[nm.o("prev_vel_2"), scen[s]] = f[nm.o("vel_z"), scen[s]] + 0.2
    noise[scen["tumble29"]] = 0.0
    # the setpoint 50 m below: thrust <= 0
    cf[2, scen["target_below"]] = (f[nm.o("pos_z"), scen["target_below"]] - 50.0).astype(np.float32)
    # poses: at rest, equal motor speeds (no torque, so the sub-step keeps the attitude), prev_rpy at the pose
    eps = 5e-7
    poses = {"pitch_up": (0.0, math.pi / 2 - eps, 0.3), "pitch_down": (0.0, -(math.pi / 2 - eps), -0.4),
             "yaw_seam": (0.02, -0.03, math.pi - 1e-7), "yaw_seam_crossed": (0.02, -0.03, -(math.pi - 1e-7))}
    for s, rpy in poses.items():
        c = scen[s]
        q = O.quat_from_euler(np.array(rpy))
        back = O.euler_from_quat(q)
        put(("quat_x", "quat_y", "quat_z", "quat_w"), c, q)
        put(("link_quat_x", "link_quat_y", "link_quat_z", "link_quat_w"), c, q)
        for grp in ("omega", "angv", "vel"):
            put([f"{grp}_{a}" for a in "xyz"], c, (0.0, 0.0, 0.0))
        put([f"prev_vel_{k}" for k in range(3)], c, (0.0, 0.0, 0.0))
        put([f"prev_rpy_{k}" for k in range(3)], c, back)
        put([f"rpm_{k}" for k in range(4)] + [f"prev_rpm_{k}" for k in range(4)], c, [14000.0] * 8)
    # the last yaw on the other side of the seam: the wrapper's rate is 2 pi / dt, the moments saturate
    f[nm.o("prev_rpy_2"), scen["yaw_seam_crossed"]] = math.pi - 1e-7
    # at pitch +-pi/2 the body z axis lies along world +-x (yaw 0.3 / -0.4): a setpoint 5 m that way keeps the
    # thrust clearly positive instead of on the sign's edge
    for s, sx in (("pitch_up", 1.0), ("pitch_down", -1.0)):
        c = scen[s]
        yaw = poses[s][2]
        cf[0, c] = (f[nm.o("pos_x"), c] + sx * 5.0 * math.cos(yaw)).astype(np.float32)
        cf[1, c] = (f[nm.o("pos_y"), c] + sx * 5.0 * math.sin(yaw)).astype(np.float32)
        cf[2, c] = f[nm.o("pos_z"), c].astype(np.float32)
    # integrators at their clamps (+-2, +-2, +-0.4; +-1, +-1, +-1500)
    for s, sg in (("integrators_high", 1.0), ("integrators_low", -1.0)):
        put([f"i_err_{k}" for k in range(3)], scen[s], (2.0 * sg, 2.0 * sg, 0.4 * sg))
        put([f"i_err_m_{k}" for k in range(3)], scen[s], (1.0 * sg, 1.0 * sg, 1500.0 * sg))
    f = f32_representable(f)
    orc.set_state(f, i)
    orc.set_command_state(cf, ci)
    stats = Stats()
    (fg, ig), (fo, io) = per_call(ctl, orc, nm, precision, noise.reshape(E, N, 4), stats)
    g = lambda n: fg[nm.cf.index(n)]   # noqa: E731
    tick0 = i[nm.oi.index("tick")]
    np.testing.assert_array_equal(ig[nm.ci.index("tick")], tick0 + 1)
    # motors cut at 30: no firmware call, rpm the clamp floor
    c = scen["tumble29"]
    assert (ig[nm.ci.index("tumble")][c] == 30).all()
    for k in range(4):
        np.testing.assert_allclose(g(f"rpm_{k}")[c], RPM_FLOOR, rtol=1e-6 if precision == "fp32" else 1e-12)
    np.testing.assert_array_equal(ig[nm.ci.index("last_att_tick")][c], i[nm.oi.index("last_att_tick")][c])
    c = scen["tumble28"]
    assert (ig[nm.ci.index("tumble")][c] == 29).all()
    assert (np.max([g(f"rpm_{k}")[c] for k in range(4)], axis=0) > RPM_FLOOR + 1).all(), "motors cut one call early"
    # thrust <= 0: moments and both integrators zeroed
    c = scen["target_below"]
    assert (g("ctl_thrust")[c] <= 0).all()
    for n in ("ctl_roll", "ctl_pitch", "ctl_yaw", "i_err_0", "i_err_1", "i_err_2", "i_err_m_0", "i_err_m_1", "i_err_m_2"):
        assert (g(n)[c] == 0).all(), n
    # the gimbal branch was entered with positive thrust; at the seam the yaw moment saturates (the setpoint's yaw is
    # the hover target's, half a turn away; across the seam the wrapper's rate is 2 pi / dt on top)
    for s in ("pitch_up", "pitch_down"):
        assert (g("ctl_thrust")[scen[s]] > 0).all(), s
        assert (np.abs(fo[nm.o("prev_rpy_1"), scen[s]]) > math.pi / 2 - 1e-5).all(), s
    assert (np.abs(g("ctl_yaw")[scen["yaw_seam_crossed"]]) == 32000).all()
    for s, sg in (("integrators_high", 1.0), ("integrators_low", -1.0)):
        for n, lim in (("i_err_0", 2.0), ("i_err_1", 2.0), ("i_err_2", 0.4), ("i_err_m_0", 1.0), ("i_err_m_1", 1.0), ("i_err_m_2", 1500.0)):
            assert (np.abs(g(n)[scen[s]]) <= float(np.float32(lim))).all(), (s, n)    # (the firmware's float clamps)
    print("\n" + stats.line(f"constructed states {precision}"))
    ctl.close()


# ------------------------------------------------------------------------------------------------------------
# 5. commander
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_commander(precision):
    E, N = 4, 2
    orc, ctl, nm, rng, std = setup(E, N, precision, ticks=0)
    obs0 = orc.reset()
    stats = Stats()
    noise = lambda: rng.normal(0, std, (E, N, 4))   # noqa: E731

    def set_tick(t):
        f, i = orc.get_state()
        i[nm.oi.index("tick")] = t
        i[nm.oi.index("last_att_tick")] = t - 1
        i[nm.oi.index("last_pos_tick")] = t - 3
        orc.set_state(f, i)

    def calls(n, command=None):
        for k in range(n):
            per_call(ctl, orc, nm, precision, noise(), stats, command=command if k == 0 else None)

    def everyone(cmd, args):
        return encode_commands([[(cmd, args)] * N] * E, E, N)

    # TAKEOFF 0.5 m in 2 s: the plan runs over t = 2 .. 4 s (t_begin = args[-1], test_commander_gpu.py)
    calls(2, everyone(Command.TAKEOFF, [0.5, 2.0]))
    assert (orc.get_command_state()[1][0] == 1).all() and (orc.get_command_state()[1][1] == 0).all()
    set_tick(1500)
    calls(2)
    set_tick(1998)
    calls(4)
    # GOTO: t_begin 0 (relative = False is args[-1]), 1.5 s
    goto = encode_commands([[(Command.GOTO, [obs0[e, n, :3] + [0.2, 0.1, 0.5], 0.2, 1.5, False]) for n in range(N)]
                            for e in range(E)], E, N)
    set_tick(1)
    calls(2, goto)
    set_tick(375)
    calls(2)
    set_tick(748)
    calls(4)
    # LAND finds the planner stopped: idle, override off
    calls(2, everyone(Command.LAND, [0.0, 2.0]))
    assert (orc.get_command_state()[1][0] == 0).all() and (orc.get_command_state()[1][1] == 0).all()
    # FULLSTATE after a plan: override back on
    z = np.zeros(3)
    full = encode_commands([[(Command.FULLSTATE, [obs0[e, n, :3] + [0.1, 0, 0.6], [0.1, 0, 0.2], [0.5, 0.5, 0.5], 0.3, [0, 0, 0.2], 0.0])
                             for n in range(N)] for e in range(E)], E, N)
    calls(2, full)
    assert (ctl.get_command_state()[1][1] == 1).all()
    calls(2, everyone(Command.STOP, [0.12]))
    calls(2, everyone(Command.NOTIFY, [0.2]))
    # a mask: every other controller gets a GOTO, through the class's own send*Cmd on the handle's side
    mask = (np.arange(E * N).reshape(E, N) % 2) == 0
    args = [np.array([0.1, -0.2, 0.2]), 0.5, 1.0, True]
    f0, i0 = orc.get_state()
    f0 = f32_representable(f0)
    orc.set_state(f0, i0)
    copy_in(ctl, orc, nm, f0, i0)
    before = [t.cpu().numpy() for t in ctl.get_command_state()]
    orc.command(*pack_command(Command.GOTO, args, E, N, mask))
    ctl.sendGotoCmd(*args, mask=mask)
    after = [t.cpu().numpy() for t in ctl.get_command_state()]
    off = ~mask.reshape(-1)
    np.testing.assert_array_equal(after[0][:, off], before[0][:, off])
    np.testing.assert_array_equal(after[1][:, off], before[1][:, off])
    assert (after[1][0][~off] == 1).all() and (after[1][0][off] == 0).all()
    check_command_state(ctl, orc, precision)
    print("\n" + stats.line(f"commander {precision}"))
    ctl.close()


# ------------------------------------------------------------------------------------------------------------
# 6. reset
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_reset_matches_oracle_and_respects_mask(precision):
    E, N = 9, 8
    orc, ctl, nm, rng, std = setup(E, N, precision)
    stats = Stats()
    per_call(ctl, orc, nm, precision, rng.normal(0, std, (E, N, 4)), stats)     # the handle holds a flight state
    before = [t.cpu().numpy() for t in ctl.get_state() + ctl.get_command_state()]
    obs0 = orc.reset()
    fo, io = orc.get_state()
    cfo, cio = orc.get_command_state()
    mask = np.arange(E * N).reshape(E, N) % 3 != 1
    ctl.reset(torch.from_numpy(obs0), mask=mask)
    after = [t.cpu().numpy() for t in ctl.get_state() + ctl.get_command_state()]
    on = mask.reshape(-1)
    for a, b in zip(after, before):        # unmasked rows: bit for bit (NaN included)
        np.testing.assert_array_equal(np.ascontiguousarray(a[:, ~on]).view(np.uint8), np.ascontiguousarray(b[:, ~on]).view(np.uint8))
    want = fo[nm.fmap]
    hist = [k for k, n in enumerate(nm.cf) if n.startswith(("prev_rpy_", "prev_vel_"))]
    want[hist] = f32_representable(want[hist])          # (taken from the float32 observation rows)
    np.testing.assert_array_equal(after[0][:, on].astype(np.float64), want[:, on])
    np.testing.assert_array_equal(after[1][:, on], io[nm.imap][:, on])
    np.testing.assert_array_equal(after[3][:, on], cio[:, on])
    np.testing.assert_array_equal(after[2][:, on], cfo[:, on])
    assert np.isnan(after[0][nm.cf.index("prev_omega_roll")][on]).all()
    # a per-env mask, and the env's own rows as init_obs
    ctl.reset(torch.from_numpy(obs0), mask=np.ones(E))
    np.testing.assert_array_equal(ctl.get_state()[1].cpu().numpy(), io[nm.imap])
    ctl.close()


# ------------------------------------------------------------------------------------------------------------
# 7. compute_env
# ------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_compute_env_is_compute_on_the_handles_rows(precision):
    E, N = 9, 8
    env = CtrlAviary(num_drones=N, num_envs=E, pyb_freq=500, ctrl_freq=500, precision=precision, seed=4,
                     init_noise={"xyz": 0.2, "rpy": 0.4, "vel": 0.3, "omega": 1.0})
    env.reset()
    a = MellingerControl(num_envs=E, num_drones=N, precision=precision)
    b = MellingerControl(num_envs=E, num_drones=N, precision=precision)
    real, dev = a.real, a.device
    z = np.zeros(3)
    for c in (a, b):
        c.reset(env)
        c.sendFullStateCmd(env._obs[..., 0:3].double().cpu().numpy() + [0.1, -0.1, 0.4], z, z, 0.2, z, 0.0)
    names, _ = env.state_field_names()
    dist = torch.from_numpy(np.random.default_rng(0).normal(0, 1e-3, (E, N, 4))).to(dev, real)
    rpy = torch.zeros((E, N, 3), dtype=real, device=dev)
    for _ in range(3):
        env.step(torch.full((E, N, 4), 14000.0, device=dev))
        f = env.get_state()[0]
        pos = torch.stack([f[names.index(n)] for n in ("pos_x", "pos_y", "pos_z")], -1).reshape(E, N, 3)
        vel = torch.stack([f[names.index(n)] for n in ("vel_x", "vel_y", "vel_z")], -1).reshape(E, N, 3)
        ra = a.computeControlFromState(env.CTRL_TIMESTEP, env, disturbance=dist, rpy_out=rpy).clone()
        rb = b.computeControl(env.CTRL_TIMESTEP, pos, rpy, vel, None, dist).clone()
        np.testing.assert_array_equal(bits(ra), bits(rb))
        for x, y in zip(a.get_state() + a.get_command_state(), b.get_state() + b.get_command_state()):
            np.testing.assert_array_equal(bits(x), bits(y))
        assert torch.isfinite(ra).all() and (ra >= RPM_FLOOR - 1).all()
    # the angles are the quaternion's
    quat = torch.stack([f[names.index(n)] for n in ("quat_x", "quat_y", "quat_z", "quat_w")], -1).double().cpu().numpy()
    want = np.stack([O.euler_from_quat(q) for q in quat])
    np.testing.assert_allclose(rpy.double().cpu().numpy().reshape(-1, 3), want, rtol=0, atol=2e-6 if precision == "fp32" else 1e-12)
    # state rows [E, N, 20] in place equal three packed arrays
    c1 = MellingerControl(num_envs=E, num_drones=N, precision=precision)
    c2 = MellingerControl(num_envs=E, num_drones=N, precision=precision)
    rows = env._obs.clone()
    r1 = c1.computeControlFromState(env.CTRL_TIMESTEP, rows).clone()
    r2 = c2.computeControl(env.CTRL_TIMESTEP, rows[..., 0:3], rows[..., 7:10], rows[..., 10:13]).clone()
    np.testing.assert_array_equal(bits(r1), bits(r2))
    for c in (a, b, c1, c2):
        c.close()
    env.close()


def test_compute_env_refuses_other_tasks():
    E, N = 4, 2
    ctl = MellingerControl(num_envs=E, num_drones=N, precision="fp32")
    race = MultiRaceAviary("level0", num_drones=N, num_envs=E, precision="fp32", autoreset=False)
    with pytest.raises(ValueError, match="only CtrlAviary handles"):
        ctl.computeControlFromState(0.002, race)
    race.close()
    one = MellingerControl(num_envs=E, num_drones=1, precision="fp32")
    hover = HoverAviary(num_envs=E, precision="fp32")
    with pytest.raises(ValueError, match="only CtrlAviary handles"):
        one.computeControlFromState(0.002, hover)
    hover.close()
    env = CtrlAviary(num_drones=N, num_envs=E, precision="fp64")
    with pytest.raises(ValueError, match="the controller"):
        ctl.computeControlFromState(0.002, env)          # precision differs
    with pytest.raises(ValueError, match="the controller"):
        one.computeControlFromState(0.002, env)          # E * N differs
    with pytest.raises(ValueError, match="cur_rpy must have shape"):
        ctl.computeControl(0.002, torch.zeros(E, N, 3), torch.zeros(E, N, 4), torch.zeros(E, N, 3))
    with pytest.raises(ValueError, match="inputs must be"):
        ctl.computeControl(0.002, *(torch.zeros(E, N, 3, dtype=torch.float64),) * 3)
    env.close()
    ctl.close()
    one.close()


# ------------------------------------------------------------------------------------------------------------
# 8. closed loop
# ------------------------------------------------------------------------------------------------------------
def closed_loop(ticks=1500):
    E, N = 4, 2
    xyz = np.array([[0.0, 0.0, 1.0], [0.6, 0.3, 1.2]])
    env = CtrlAviary(DroneModel.CF2X, num_drones=N, initial_xyzs=xyz, physics=Physics.PYB, pyb_freq=500, ctrl_freq=500,
                     num_envs=E, precision="fp64")
    ctl = MellingerControl(DroneModel.CF2X, num_envs=E, num_drones=N, precision="fp64")
    env.reset()
    ctl.reset(env)
    target = xyz + [0.0, 0.0, 0.5]
    z = np.zeros(3)
    ctl.sendFullStateCmd(np.broadcast_to(target, (E, N, 3)), z, z, 0.0, z, 0.0)
    for _ in range(ticks):
        env.step(ctl.computeControlFromState(env.CTRL_TIMESTEP, env))
    obs = env._obs.double().cpu().numpy()
    ticks_done = ctl.get_state()[1][0].cpu().numpy()
    env.close()
    ctl.close()
    assert (ticks_done == ticks).all()
    return obs, target


def test_closed_loop_converges():
    """CtrlAviary + MellingerControl at 500 / 500 Hz, FULLSTATE 0.5 m above the start, 1500 ticks, to the bars of
    tests/test_race_oracle.py::test_mellinger_takeoff_converges.  CtrlAviary's body is cf2x_IROS.urdf's (0.03454 kg;
    the race drone the firmware's thrust model is tuned for weighs 0.027 kg, the other constants are equal): it
    settles 1.6 cm above the target, the lighter body 5.3 cm, both inside the bars."""
    obs, target = closed_loop()
    print(f"\n[mellinger] closed loop: |xy error| max {np.abs(obs[..., :2] - target[..., :2]).max():.4f} m, "
          f"z error {np.abs(obs[..., 2] - target[..., 2]).max():.4f} m, |roll, pitch| max {np.abs(obs[..., 7:9]).max():.4f}")
    np.testing.assert_allclose(obs[..., :2], np.broadcast_to(target[..., :2], obs[..., :2].shape), atol=0.02)
    assert (np.abs(obs[..., 2] - target[..., 2]) < 0.1).all()
    assert (np.abs(obs[..., 7:9]) < 0.05).all()
