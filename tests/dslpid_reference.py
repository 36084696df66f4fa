"""numpy float64 restatement of DSLPIDControl.computeControl (control/DSLPIDControl.py:82-259) with both
mixers, target_rpy_rates, pos_e and the yaw error, for the stand-alone controller's tests.

It follows the kernel's conventions, not the reference's call sequence: the scipy Euler round trip of the
target rotation is skipped (the identity on a proper rotation), the yaw error's first term is the third
angle of the intrinsic 'XYZ' decomposition of the target basis T = Rx(a) Ry(b) Rz(c), c = atan2(-T01, T00),
and the current Euler angles are pybullet's getEulerFromQuaternion away from gimbal lock.
tests/test_dslpid.py pins it to the reference's own outputs (tests/golden/dslpid_golden.npz,
pid_golden.npz) at 1e-9.
"""
import os

import numpy as np

MIXERS = {"cf2x": np.array([[-.5, -.5, -1], [-.5, .5, 1], [.5, .5, -1], [.5, -.5, 1]]),
          "cf2p": np.array([[0., -1, -1], [1, 0, 1], [0, 1, -1], [-1, 0, 1]])}
MASS = {"cf2x": 0.03454, "cf2p": 0.027}      # cf2x_IROS.urdf, cf2p.urdf
KF = 3.16e-10
DEFAULT_GAINS = dict(p_for=[.4, .4, 1.25], i_for=[.05, .05, .05], d_for=[.2, .2, .5],
                     p_tor=[70000., 70000., 60000.], i_tor=[.0, .0, 500.], d_tor=[20000., 20000., 12000.])
PWM2RPM_SCALE, PWM2RPM_CONST, MIN_PWM, MAX_PWM = 0.2685, 4070.3, 20000.0, 65535.0


def rot_matrix(q):
    """[K, 4] xyzw unit quaternions -> [K, 3, 3] body-to-world"""
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def euler_xyz(q):
    """getEulerFromQuaternion (extrinsic x-y-z) on [K, 4] xyzw, generic branch"""
    x, y, z, w = q.T
    sarg = -2 * (x * z - w * y)
    assert (np.abs(sarg) < 0.99999).all(), "gimbal lock is outside this restatement"
    return np.stack([np.arctan2(2 * (y * z + w * x), w * w - x * x - y * y + z * z), np.arcsin(sarg),
                     np.arctan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z)], -1)


class Controller:
    """K controllers; state [K, 9] = last_rpy 3, integral_pos_e 3, integral_rpy_e 3"""

    def __init__(self, K, mixer="cf2x", g=9.8, gains=None):
        self.K = K
        self.mixer = MIXERS[mixer]
        self.gravity = g * MASS[mixer]
        self.kf = KF
        self.gains = {k: np.array(v, float) for k, v in DEFAULT_GAINS.items()}
        if gains:
            self.gains.update({k: np.array(v, float) for k, v in gains.items()})
        self.state = np.zeros((K, 9))

    def compute(self, dt, pos, quat, vel, target_pos, target_rpy=None, target_vel=None, target_rpy_rates=None):
        """[K, .] float64 inputs -> rpm [K, 4], pos_e [K, 3], yaw_e [K]; the state advances"""
        K, G = self.K, self.gains
        zeros = np.zeros((K, 3))
        target_rpy = zeros if target_rpy is None else np.broadcast_to(target_rpy, (K, 3))
        target_vel = zeros if target_vel is None else np.broadcast_to(target_vel, (K, 3))
        rates = zeros if target_rpy_rates is None else np.broadcast_to(target_rpy_rates, (K, 3))
        R = rot_matrix(quat)
        rpy = euler_xyz(quat)
        last_rpy, int_pos, int_rpy = self.state[:, 0:3], self.state[:, 3:6], self.state[:, 6:9]
        pos_e = np.broadcast_to(target_pos, (K, 3)) - pos
        vel_e = target_vel - vel
        int_pos = np.clip(int_pos + pos_e * dt, -2., 2.)
        int_pos[:, 2] = np.clip(int_pos[:, 2], -0.15, .15)
        tt = G["p_for"] * pos_e + G["i_for"] * int_pos + G["d_for"] * vel_e + np.array([0, 0, self.gravity])
        scalar = np.maximum(0., np.einsum("ki,ki->k", tt, R[:, :, 2]))
        thrust = (np.sqrt(scalar / (4 * self.kf)) - PWM2RPM_CONST) / PWM2RPM_SCALE
        z_ax = tt / np.linalg.norm(tt, axis=1, keepdims=True)
        x_c = np.stack([np.cos(target_rpy[:, 2]), np.sin(target_rpy[:, 2]), np.zeros(K)], -1)
        y_c = np.cross(z_ax, x_c)
        y_ax = y_c / np.linalg.norm(y_c, axis=1, keepdims=True)
        x_ax = np.cross(y_ax, z_ax)
        Rt = np.stack([x_ax, y_ax, z_ax], -1)                # columns
        yaw_e = np.arctan2(-Rt[:, 0, 1], Rt[:, 0, 0]) - rpy[:, 2]
        Me = np.einsum("kji,kjl->kil", Rt, R) - np.einsum("kji,kjl->kil", R, Rt)
        rot_e = np.stack([Me[:, 2, 1], Me[:, 0, 2], Me[:, 1, 0]], -1)
        rates_e = rates - (rpy - last_rpy) / dt
        int_rpy = np.clip(int_rpy - rot_e * dt, -1500., 1500.)
        int_rpy[:, 0:2] = np.clip(int_rpy[:, 0:2], -1., 1.)
        tq = np.clip(-G["p_tor"] * rot_e + G["d_tor"] * rates_e + G["i_tor"] * int_rpy, -3200, 3200)
        pwm = np.clip(thrust[:, None] + tq @ self.mixer.T, MIN_PWM, MAX_PWM)
        self.state = np.concatenate([rpy, int_pos, int_rpy], 1)
        return PWM2RPM_SCALE * pwm + PWM2RPM_CONST, pos_e, yaw_e


# ---------------------------------------------------------------------------------------------
# the fixture (tests/golden/dslpid_golden.npz, tests/golden/make_dslpid_golden.py) and the tests' bar
# ---------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dslpid_golden.npz")
MIXER_OF = {"x": "cf2x", "p": "cf2p"}
STATE_GROUPS = ("pid_last_rpy", "pid_int_pos", "pid_int_rpy")
GAIN_KEYS = {"p_for": "p_coeff_pos", "i_for": "i_coeff_pos", "d_for": "d_coeff_pos",
             "p_tor": "p_coeff_att", "i_tor": "i_coeff_att", "d_tor": "d_coeff_att"}


def load():
    return np.load(GOLDEN)


def fixture_gains(fx, keyword=False):
    """the non-default gains of the fixture's last eight sequences, keyed as Controller takes them or by
    setPIDCoefficients' keywords"""
    return {(kw if keyword else k): fx["gains_" + kw] for k, kw in GAIN_KEYS.items()}


def vec_err(got, want, floor):
    """per row |got - want| / max(|want|, floor), 2-norms over the vector's components ([K, c] or [K] arrays)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.ndim == 1:
        got, want = got[:, None], want[:, None]
    return np.linalg.norm(got - want, axis=-1) / np.maximum(np.linalg.norm(want, axis=-1), floor)


def output_errors(rpm, pos_e, yaw_e, state, want_rpm, want_pos_e, want_yaw_e, want_state):
    """{name: per-row error} of the three outputs and the three state vectors (state [K, 9])"""
    errs = {"rpm": vec_err(rpm, want_rpm, 1.0), "pos_e": vec_err(pos_e, want_pos_e, 1e-3), "yaw_e": vec_err(yaw_e, want_yaw_e, 1e-3)}
    for k, g in enumerate(STATE_GROUPS):
        errs[g] = vec_err(state[:, 3 * k:3 * k + 3], want_state[:, 3 * k:3 * k + 3], 1e-3)
    return errs


def assert_outputs(rpm, pos_e, yaw_e, state, want_rpm, want_pos_e, want_yaw_e, want_state, rtol, what=""):
    for name, err in output_errors(rpm, pos_e, yaw_e, state, want_rpm, want_pos_e, want_yaw_e, want_state).items():
        assert err.max() <= rtol, f"{what}{name}: max rel err {err.max():.3e} (row {err.argmax()})"


def loop_rows_before(fx, case, t):
    """[N, 23] the rows the env held before step t of a pid.py loop (row + rpy_rates; zero rates at the start)"""
    if t > 0:
        return np.concatenate([fx[f"{case}_obs"][t - 1], fx[f"{case}_rpy_rates"][t - 1]], -1)
    init = fx[f"{case}_init"]
    return np.concatenate([init, np.zeros((init.shape[0], 3))], -1)


def loop_rows_after(fx, case, t):
    return np.concatenate([fx[f"{case}_obs"][t], fx[f"{case}_rpy_rates"][t]], -1)


def loop_ctl_before(fx, case, t):
    """[N, 9] the controllers' state before the call that follows step t"""
    return fx[f"{case}_ctl"][t - 1].copy() if t > 0 else np.zeros_like(fx[f"{case}_ctl"][0])


def loop_action(fx, case, t):
    """[N, 4] the RPMs of step t: zeros first, then what the controllers returned after step t - 1"""
    return fx[f"{case}_rpm"][t - 1] if t > 0 else np.zeros_like(fx[f"{case}_rpm"][0])
