"""Shared by the CtrlAviary / VelocityAviary tests: the fixture (tests/golden/ctrl_golden.npz, the
reference's own episodes, tests/golden/make_ctrl_golden.py) and its mapping onto the state snapshot.

A reference row is ``_getDroneStateVector``: pos 0:3, quat 3:7 (xyzw), rpy 7:10, vel 10:13, ang_v 13:16,
last_clipped_action 16:20.  Under Physics.DYN the snapshot's ``omega_*`` is the body-frame rpy_rates, which
the row does not hold: the fixture stores them beside it.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctrl_golden.npz")
CTRL_CASES = [(f"c{N}s{S}", N, S) for N in (1, 2, 3) for S in (5, 1)]
VEL_CASES = [("v2s5", 2, 5), ("v3s5", 3, 5)]
PID_NAMES = ["pid_last_rpy_x", "pid_last_rpy_y", "pid_last_rpy_z", "pid_int_pos_x", "pid_int_pos_y", "pid_int_pos_z",
             "pid_int_rpy_x", "pid_int_rpy_y", "pid_int_rpy_z"]
# state vectors of a DYN step and where the reference row (+ rpy_rates at 20:23) holds them
DYN_GROUPS = (("pos", slice(0, 3)), ("quat", slice(3, 7)), ("vel", slice(10, 13)), ("omega", slice(20, 23)),
              ("angv", slice(13, 16)), ("last_rpm", slice(16, 20)))


def load():
    return np.load(GOLDEN)


def rows_before(fx, case, t):
    """[EP, N, 23] what the reference held before step t: row + rpy_rates (the start state has zero
    rates and zero RPMs)"""
    if t > 0:
        return np.concatenate([fx[f"{case}_obs"][:, t - 1], fx[f"{case}_rpy_rates"][:, t - 1]], -1)
    init = fx[f"{case}_init"]                      # pos 3, quat 4, vel 3, ang 3
    EP, N = init.shape[:2]
    r = np.zeros((EP, N, 23))
    r[..., 0:7] = init[..., 0:7]
    r[..., 10:13] = init[..., 7:10]
    return r


def rows_after(fx, case, t):
    return np.concatenate([fx[f"{case}_obs"][:, t], fx[f"{case}_rpy_rates"][:, t]], -1)


def ctl_before(fx, case, t):
    """[EP, N, 9] the controllers' state before step t"""
    return fx[f"{case}_ctl"][:, t - 1] if t > 0 else fx[f"{case}_ctl0"]


def fill_state(names, rows, ctl=None):
    """state snapshot [nf, K] (float64) from K rows [K, 23]; link_quat = quat"""
    idx = {n: k for k, n in enumerate(names)}
    f = np.zeros((len(names), rows.shape[0]))
    for k, ax in enumerate("xyz"):
        f[idx[f"pos_{ax}"]] = rows[:, k]; f[idx[f"vel_{ax}"]] = rows[:, 10 + k]
        f[idx[f"omega_{ax}"]] = rows[:, 20 + k]; f[idx[f"angv_{ax}"]] = rows[:, 13 + k]
    for k, ax in enumerate("xyzw"):
        f[idx[f"quat_{ax}"]] = rows[:, 3 + k]; f[idx[f"link_quat_{ax}"]] = rows[:, 3 + k]
    for k in range(4):
        f[idx[f"last_rpm_{k}"]] = rows[:, 16 + k]
    if ctl is not None:
        for k, nme in enumerate(PID_NAMES):
            f[idx[nme]] = ctl[:, k]
    return f


def vec_err(got, want, floor):
    """per column |got - want| / max(|want|, floor), 2-norms over the vector's components ([K, c] arrays)"""
    return np.linalg.norm(got - want, axis=-1) / np.maximum(np.linalg.norm(want, axis=-1), floor)
