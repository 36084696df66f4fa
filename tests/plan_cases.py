"""The pinned sample of the spline planner's tests (tests/test_plan.py, tests/test_plan_gpu.py,
tools/plan_parity.py) and the helpers they share: running csrc/plan_host, the scipy yardstick, and the
observation rows a case is planned from.

Case i of ``np.random.default_rng(1)``: ``uniform(-0.15, 0.15, (4, 3))`` added to the nominal gates' x, y, z,
then ``uniform(-0.1, 0.1, 2)`` added to start ``i % 8`` of the eight nominal drone starts (envs/tracks.py);
both rounded through float32, as an observation row carries them."""
import os
import subprocess

import numpy as np

from gym_pybullet_adrp_amd.envs import tracks
from gym_pybullet_adrp_amd.hardcoded import CTRL_FREQ, DURATION, waypoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym_pybullet_adrp_amd", "csrc")
PLAN_HOST = os.path.join(ROOT, "gym_pybullet_adrp_amd", "plan_host")
L = int(DURATION * CTRL_FREQ)
NT, NC = 20, 16          # knots / coefficients per coordinate a 16-point fit can have
SAMPLE_SIZE = 4000

GATES = np.array([[g[0], g[1], g[2], g[5]] for g in tracks._BASE["gates"]], np.float64)      # x, y, z, yaw
STARTS = np.array([tracks._BASE["init_states"][d]["pos"][:2] for d in ("drone0", "drone1")]
                  + [p[:2] for p in tracks.EXTRA_DRONES], np.float64)


def sample(count=SAMPLE_SIZE):
    """(start [count, 2], gates [count, 4, 4]) float64 holding float32 values"""
    rng = np.random.default_rng(1)
    start, gates = np.empty((count, 2)), np.empty((count, 4, 4))
    for i in range(count):
        g = GATES.copy()
        g[:, :3] += rng.uniform(-0.15, 0.15, (4, 3))
        s = STARTS[i % 8] + rng.uniform(-0.1, 0.1, 2)
        gates[i] = g.astype(np.float32).astype(np.float64)
        start[i] = s.astype(np.float32).astype(np.float64)
    return start, gates


def obs_rows(start, gates, width=49, fill=0.0):
    """float32 observation rows [count, width] with the start in [0:2] and the gates in [12:28]"""
    o = np.full((len(start), width), fill, np.float32)
    o[:, 0:2] = start
    o[:, 12:28] = np.asarray(gates).reshape(len(start), 16)
    return o


def build_plan_host():
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_host"])
    return PLAN_HOST


def run_plan_host(start, gates, tmpdir, samples=None):
    """csrc/plan_host on the cases: dict of n [C], status [C], t [C, 20], c [C, 3, 16], ref [C, L, 3]"""
    exe = build_plan_host()
    samples = np.linspace(0, 1, L) if samples is None else np.asarray(samples, np.float64)
    C, ls = len(start), len(samples)
    cases = np.concatenate([np.asarray(start, np.float64), np.asarray(gates, np.float64)[:, :, :2].reshape(C, 8)], 1)
    fin, fs, fout = (os.path.join(str(tmpdir), n) for n in ("plan_cases.f64", "plan_samples.f64", "plan_out.bin"))
    cases.tofile(fin)
    samples.tofile(fs)
    subprocess.check_call([exe, fin, fs, fout])
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == C * (8 + 8 * (NT + 3 * NC + 3 * ls))
    out, at = {}, 0
    for name, dt, shape in (("n", np.int32, (C,)), ("status", np.int32, (C,)), ("t", np.float64, (C, NT)),
                            ("c", np.float64, (C, 3, NC)), ("ref", np.float64, (C, ls, 3))):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = raw[at:at + size].view(dt).reshape(shape)
        at += size
    return out


def scipy_plan(start, gates, samples=None):
    """scipy's splprep(s = 0.1) / splev on the same cases: n [C], t [C, 20] and c [C, 3, 16] zero-padded, ref [C, L, 3]"""
    from scipy import interpolate
    samples = np.linspace(0, 1, L) if samples is None else samples
    C = len(start)
    n, t, c, ref = np.zeros(C, np.int32), np.zeros((C, NT)), np.zeros((C, 3, NC)), np.empty((C, len(samples), 3))
    for i in range(C):
        w = waypoints(start[i], gates[i])
        (ti, ci, _), _ = interpolate.splprep([w[:, 0], w[:, 1], w[:, 2]], s=0.1)
        n[i] = len(ti)
        t[i, :len(ti)] = ti
        for d in range(3):
            c[i, d, :len(ti) - 4] = ci[d][:len(ti) - 4]
        ref[i] = np.stack(interpolate.splev(samples, (ti, ci, 3)), -1)
    return {"n": n, "t": t, "c": c, "ref": ref}


# plan_host against scipy over the whole sample (tools/plan_parity.py, profiles/plan_parity.json): the largest
# coefficient / sample difference.  The tests' absolute tolerance is ten times it: the p-iteration stops at
# |f(p) - s| < 1e-4, so a last-bit difference early in it is amplified.
PARITY_MAX = 3.589251118540915e-10
ATOL = 10 * PARITY_MAX
KNOT_ATOL = 1e-14        # u is at most 15 rounded additions and one division in [0, 1]
