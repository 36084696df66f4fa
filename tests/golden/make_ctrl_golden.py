"""Generate tests/golden/ctrl_golden.npz from the reference's own CtrlAviary and VelocityAviary.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ctrl_golden.py [<path of the reference checkout>]

The reference (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08) is imported at run time under the
stand-ins of make_golden.py (pybullet as a pose store, gymnasium, munch) and never copied: both envs run
short episodes through the reference's own ``step`` with ``Physics.DYN`` (which needs no Bullet
integration).  Only data is written: the start states, the actions and what the reference returned and
held per step.

Cases: CtrlAviary with N = 1, 2, 3 drones at 240/48 Hz (5 sub-steps, ``c{N}s5``) and at the default
240/240 Hz (1 sub-step, ``c{N}s1``); VelocityAviary with N = 2, 3 at 240/48 Hz (``v{N}s5``).  2 episodes of
20 steps each (the float64 rows do not compress: more would pass the 200 KB the fixture may take) from
states near hover with a small tilt.

CtrlAviary actions: ``rpm = HOVER_RPM * (1 + 0.05 a)`` from a stored float32 ``a`` as BaseRLAviary.py:192
computes it (float32 gain, float64 product), so that the project's single-drone oracle (act=RPM) can be
driven with ``a``.  Some rows have |a| large enough for RPMs below 0 and above MAX_RPM, which CtrlAviary
clips (the oracle's RPM action type does not: those rows are marked by ``*_clipped``).
VelocityAviary actions: float32 in the action box, with zero-direction rows and rows with a3 = 0.  The
direction components are multiples of 1/64: the reference takes their norm in float32 through NumPy's
BLAS dot product, whose rounding of the sum of squares depends on the BLAS build (tests/test_pid_golden.py
meets it as a 1-ulp float32 difference in about one call of fifteen, 1e-7 relative in the target velocity).
With at most 7 significant bits per component the squares and their sum are exact in float32 in any order,
so the fixture holds the same numbers on every machine and the 1e-9 bar of the tests applies to every row.
The reference never ends an episode here and builds its DSLPID controllers once: they carry across the
episodes of a case.
"""
import importlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference, install_stubs, random_state, set_drone_state  # noqa: E402

T, N_EP = 20, 2


def start(pb, env, rng, ep):
    """drones near hover, 0.5 m apart in height about z = 1, small tilt and speed; returns [N, 13]"""
    N = env.NUM_DRONES
    init = np.zeros((N, 13))
    env.reset()
    for n in range(N):
        center = np.array([env.INIT_XYZS[n][0], env.INIT_XYZS[n][1], 1.0 + 0.3 * n])
        pos, quat, vel, _ = random_state(rng, center=center, tilt=0.05)
        pos = center + 0.2 * (pos - center)
        vel = 0.2 * vel
        set_drone_state(pb, env, n, pos, quat, vel, np.zeros(3))
        init[n] = np.concatenate([pos, quat, vel, np.zeros(3)])
    env._updateAndStoreKinematicInformation()      # _preprocessAction / _dynamics read the stored state
    env.rpy_rates[:] = 0
    return init


def run(pb, env, rng, acts, to_action, ctrl=None):
    """acts [N_EP, T, N, 4] float32 -> what the reference returned and held per step"""
    N = env.NUM_DRONES
    init = np.zeros((N_EP, N, 13))
    obs = np.zeros((N_EP, T, N, 20)); rates = np.zeros((N_EP, T, N, 3))
    rew = np.zeros((N_EP, T)); term = np.zeros((N_EP, T), bool); trunc = np.zeros((N_EP, T), bool)
    answer = np.zeros((N_EP, T), np.int64); counter = np.zeros((N_EP, T), np.int64)
    ctl0 = np.zeros((N_EP, N, 9)); ctl = np.zeros((N_EP, T, N, 9))

    def ctl_state():
        return np.array([np.concatenate([c.last_rpy, c.integral_pos_e, c.integral_rpy_e]) for c in ctrl])
    for ep in range(N_EP):
        init[ep] = start(pb, env, rng, ep)
        c0 = env.step_counter
        if ctrl:
            ctl0[ep] = ctl_state()
        for t in range(T):
            o, r, te, tr, info = env.step(to_action(acts[ep, t]))
            assert np.asarray(o).shape == (N, 20) and np.asarray(o).dtype == np.float64
            obs[ep, t] = o; rates[ep, t] = env.rpy_rates
            rew[ep, t] = r; term[ep, t] = te; trunc[ep, t] = tr; answer[ep, t] = info["answer"]
            counter[ep, t] = env.step_counter - c0
            if ctrl:
                ctl[ep, t] = ctl_state()
    d = dict(init=init, act=acts, obs=obs, rpy_rates=rates, rew=rew, term=term, trunc=trunc, answer=answer,
             counter=counter, init_xyzs=np.array(env.INIT_XYZS, float),
             obs_low=env.observation_space.low.astype(np.float32), obs_high=env.observation_space.high.astype(np.float32),
             act_low=env.action_space.low.astype(np.float32), act_high=env.action_space.high.astype(np.float32))
    if ctrl:
        d.update(ctl0=ctl0, ctl=ctl)
    return d


def main():
    os.chdir(REF)
    pb = install_stubs()
    m = import_reference(pb)
    CA = importlib.import_module("gym_pybullet_adrp.envs.CtrlAviary")
    VA = importlib.import_module("gym_pybullet_adrp.envs.VelocityAviary")
    E = m.enums
    fx = {}
    for N in (1, 2, 3):
        for S in (5, 1):
            rng = np.random.default_rng(700 + 10 * N + S)
            env = CA.CtrlAviary(num_drones=N, physics=E.Physics.DYN, pyb_freq=240, ctrl_freq=240 // S)
            assert env.PYB_STEPS_PER_CTRL == S
            acts = rng.uniform(-1, 1, (N_EP, T, N, 4)).astype(np.float32)
            # clip rows: motors below 0 (a < -20) and above MAX_RPM = 1.5 HOVER_RPM (a > 10)
            acts[0, 3, 0, 1] = -26.0
            acts[0, 3, N - 1, 2] = 13.5
            acts[1, 11, N - 1] = np.float32([-21.0, 12.0, 30.0, -40.0])

            def to_rpm(a, env=env):
                return env.HOVER_RPM * (1 + np.float32(0.05) * a)    # float32 gain, float64 product
            assert to_rpm(acts[0, 0]).dtype == np.float64 and (1 + np.float32(0.05) * acts[0, 0]).dtype == np.float32
            d = run(pb, env, rng, acts, to_rpm)
            rpm = np.array([[to_rpm(acts[ep, t]) for t in range(T)] for ep in range(N_EP)])
            d["clipped"] = ((rpm < 0) | (rpm > env.MAX_RPM)).any(-1)          # [N_EP, T, N]
            assert (rpm < 0).any() and (rpm > env.MAX_RPM).any(), "the fixture needs rows clipped at both ends"
            np.testing.assert_array_equal(d["obs"][..., 16:20], np.clip(rpm, 0, env.MAX_RPM))
            assert not d["term"].any() and not d["trunc"].any() and (d["rew"] == -1).all() and (d["answer"] == 42).all()
            fx.update({f"c{N}s{S}_{k}": v for k, v in d.items()})
            fx["MAX_RPM"], fx["HOVER_RPM"] = np.float64(env.MAX_RPM), np.float64(env.HOVER_RPM)
            print(f"c{N}s{S}", "steps", N_EP * T, "clipped drone-steps", int(d["clipped"].sum()))
    for N in (2, 3):
        rng = np.random.default_rng(800 + N)
        env = VA.VelocityAviary(num_drones=N, physics=E.Physics.DYN, pyb_freq=240, ctrl_freq=48)
        acts = rng.uniform(-1, 1, (N_EP, T, N, 4)).astype(np.float32)
        acts[..., 3] = np.abs(acts[..., 3])
        acts[..., :3] = np.round(acts[..., :3] * 64) / 64    # exact float32 sum of squares (docstring)
        acts[:, ::6, 0, :3] = 0            # zero direction -> zero target velocity
        acts[:, 4::7, N - 1, 3] = 0        # zero speed fraction
        low, high = env.action_space.low, env.action_space.high
        assert ((acts >= low) & (acts <= high)).all()
        assert (acts[..., :3] == 0).all(-1).any() and (acts[..., 3] == 0).any()
        d = run(pb, env, rng, acts, lambda a: a, ctrl=env.ctrl)
        assert not d["term"].any() and not d["trunc"].any() and (d["rew"] == -1).all() and (d["answer"] == 42).all()
        fx.update({f"v{N}s5_{k}": v for k, v in d.items()})
        fx["SPEED_LIMIT"] = np.float64(env.SPEED_LIMIT)
        print(f"v{N}s5", "steps", N_EP * T, "max tilt", float(np.abs(d["obs"][..., 7:9]).max()))
    # the default constructors (240 / 240 Hz, one drone) and the default formation of three
    env = CA.CtrlAviary(num_drones=3)
    fx["INIT_XYZS"] = np.array(env.INIT_XYZS, float)
    fx["default_freqs"] = np.array([CA.CtrlAviary().PYB_FREQ, CA.CtrlAviary().CTRL_FREQ, VA.VelocityAviary().PYB_FREQ,
                                    VA.VelocityAviary().CTRL_FREQ, CA.CtrlAviary().NUM_DRONES, VA.VelocityAviary().NUM_DRONES])
    path = os.path.join(HERE, "ctrl_golden.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print("wrote", path, len(fx), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
