"""Generate tests/golden/multihover_golden.npz from the reference's own MultiHoverAviary.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_multihover_golden.py [<path of the reference checkout>]

The reference (FelixWaiblinger/gym-pybullet-adrp @ 2024-10-08) is imported at run time under the
stand-ins of make_golden.py (pybullet as a pose store, gymnasium, munch) and never copied:
``MultiHoverAviary(physics=DYN, act=RPM)`` and ``act=ONE_D_RPM`` run whole episodes through the
reference's own ``step`` (Physics.DYN needs no Bullet integration).  Only data is written: the start
states, the actions and what the reference returned per step.

Cases: N = 2 and N = 3 drones at the default INIT_XYZS with RPM actions (3 episodes each), N = 2 with
ONE_D_RPM (2 episodes): 8 episodes of 40 steps (the float64 states do not compress: more would pass
the 200 KB the fixture may take) from states near the targets with a small tilt; episode 1 of a case
starts tilted and episode 2 next to the position bound, so that the fixture holds truncated steps of
both kinds (asserted below).
The reference does not reset on truncation: an episode runs on, so truncated and non-truncated steps
alternate within one episode.
"""
import importlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference, install_stubs, random_state, set_drone_state  # noqa: E402

T = 40


def episodes(pb, m, MH, N, act_type, A, seed, N_EP):
    E = m.enums
    rng = np.random.default_rng(seed)
    env = MH.MultiHoverAviary(num_drones=N, physics=E.Physics.DYN, act=act_type)
    B = env.ACTION_BUFFER_SIZE
    D = 12 + B * A
    init = np.zeros((N_EP, N, 13)); acts = rng.uniform(-1, 1, (N_EP, T, N, A)).astype(np.float32)
    ring0 = np.zeros((N_EP, B, N, A), np.float32)
    obs = np.zeros((N_EP, T, N, D), np.float32); rew = np.zeros((N_EP, T)); term = np.zeros((N_EP, T), bool)
    trunc = np.zeros((N_EP, T), bool)
    state = np.zeros((N_EP, T, N, 16))      # pos 3, quat 4 (xyzw), vel 3, rpy_rates 3 (body), ang_v 3 (world)
    counter = np.zeros((N_EP, T), np.int64)  # step_counter after the step
    tilt_trunc = pos_trunc = 0
    for ep in range(N_EP):
        env.reset()
        for n in range(N):
            tilt = 0.05
            center = env.TARGET_POS[n] * np.array([1, 1, 1.0])
            pos, quat, vel, _ = random_state(rng, center=center, tilt=tilt)
            pos = center + 0.2 * (pos - center)          # within 0.1 m of the target
            vel = 0.2 * vel
            if ep == 1 and n == 0:                       # starts tilted beyond 0.4 rad roll, inside the bounds
                quat = np.array(pb.getQuaternionFromEuler([0.47, 0.02, 0.1]))
            if ep == 2 and n == N - 1:                   # starts next to the |x| bound, moving out, upright
                pos = np.array([1.97, center[1], center[2]])
                vel = np.array([0.4, 0.0, 0.0])
                quat = np.array(pb.getQuaternionFromEuler([0.0, 0.0, 0.0]))
            set_drone_state(pb, env, n, pos, quat, vel, np.zeros(3))
            init[ep, n] = np.concatenate([pos, quat, vel, np.zeros(3)])
        env._updateAndStoreKinematicInformation()
        env.rpy_rates[:] = 0
        ring0[ep] = np.array([np.asarray(a, np.float32).reshape(N, A) for a in env.action_buffer])
        for t in range(T):
            a = acts[ep, t]
            if ep == 2:
                a = acts[ep, t] = (0.2 * a).astype(np.float32)   # gentle: the drone stays upright while it drifts out
            o, r, te, tr, _ = env.step(a)
            obs[ep, t] = o; rew[ep, t] = r; term[ep, t] = te; trunc[ep, t] = tr
            state[ep, t] = np.hstack([env.pos, env.quat, env.vel, env.rpy_rates, env.ang_v])
            counter[ep, t] = env.step_counter
            if tr:
                tilted = (np.abs(env.rpy[:, :2]) > 0.4).any()
                out = (np.abs(env.pos[:, :2]) > 2.0).any() or (env.pos[:, 2] > 2.0).any()
                tilt_trunc += bool(tilted and not out)
                pos_trunc += bool(out and not tilted)
    return dict(init=init, ring0=ring0, act=acts, obs=obs, rew=rew, term=term, trunc=trunc, state=state,
                counter=counter, target=np.array(env.TARGET_POS, float), init_xyzs=np.array(env.INIT_XYZS, float),
                obs_low=env.observation_space.low.astype(np.float32), obs_high=env.observation_space.high.astype(np.float32),
                act_low=env.action_space.low.astype(np.float32), act_high=env.action_space.high.astype(np.float32)), \
        tilt_trunc, pos_trunc


def main():
    os.chdir(REF)
    pb = install_stubs()
    m = import_reference(pb)
    MH = importlib.import_module("gym_pybullet_adrp.envs.MultiHoverAviary")
    E = m.enums
    fx = {}
    tilt_all = pos_all = 0
    for name, N, at, A, seed, n_ep in (("rpm2", 2, E.ActionType.RPM, 4, 51, 3), ("rpm3", 3, E.ActionType.RPM, 4, 52, 3),
                                       ("one2", 2, E.ActionType.ONE_D_RPM, 1, 53, 2)):
        d, tilt_trunc, pos_trunc = episodes(pb, m, MH, N, at, A, seed, n_ep)
        tr = d["trunc"]
        assert tr.any() and not tr.all(), f"{name}: the fixture needs truncated and non-truncated steps"
        assert tilt_trunc >= 1, f"{name}: no truncation by tilt alone"
        assert pos_trunc >= 1 or n_ep < 3, f"{name}: no truncation by position alone"
        tilt_all += tilt_trunc
        pos_all += pos_trunc
        print(name, "steps", tr.size, "truncated", int(tr.sum()), "by tilt alone", tilt_trunc, "by position alone",
              pos_trunc, "terminated", int(d["term"].sum()))
        fx.update({f"{name}_{k}": v for k, v in d.items()})
    assert tilt_all >= 1 and pos_all >= 1
    path = os.path.join(HERE, "multihover_golden.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print("wrote", path, len(fx), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
