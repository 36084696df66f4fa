"""The hover sub-step chain carries the angular velocity in the body frame: checks of
what that reformulation could break, against the world-frame CPU oracle.  Needs an MI355X: -m gpu.

Fast spin is the case the identity wb' = wb + dt I^-1 rhs does not cover by itself: Bullet clamps the
WORLD coordinates of omega to +-100, so past |omega| = 100 the chain goes through R wb, the clamp and
R^T again, per lane.  Every wave here mixes slow envs with the three kinds of fast ones (norm above
100 with no coordinate above it, one coordinate above, all above).  Bars: the suite's, 1e-4 (fp32)
and 1e-9 (fp64) of max(|x|, floor) per state vector.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.utils.enums import Physics  # noqa: E402

from test_hover_gpu import active_fields, compare_state, pair, random_states  # noqa: E402

FAST = np.array([[70.0, 70.0, 70.0], [140.0, 20.0, -5.0], [-130.0, 110.0, 160.0]])


def spin_mix(rng, f, names):
    """overwrite omega of envs 1, 2, 3 (mod 4) with the three fast kinds (+-5 %, random signs); envs
    0 (mod 4) keep their slow omega: every wave holds all four kinds"""
    w = [names.index(f"omega_{a}") for a in "xyz"]
    E = f.shape[1]
    for e in range(E):
        if e % 4:
            f[w, e] = FAST[e % 4 - 1] * rng.uniform(0.95, 1.05) * rng.choice([-1.0, 1.0], 3)
    return f


def seed_both(env, orc, f, i):
    real = np.float64 if env.cfg.precision else np.float32
    f = f.astype(real).astype(np.float64)
    orc.set_state(f, i)
    env.set_state(torch.from_numpy(f.astype(real)), torch.from_numpy(i))
    return f


def teacher_forced(env, orc, rng, E, rtol, active, steps=3):
    worst = {}
    for _ in range(steps):
        act = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
        orc.step(act)
        env.step(torch.from_numpy(act))
        torch.cuda.synchronize()
        for g, v in compare_state(env, orc, rtol, active).items():
            worst[g] = max(worst.get(g, 0.0), v)
        seed_both(env, orc, *orc.get_state())
    print("worst relative errors:", {g: f"{v:.2e}" for g, v in sorted(worst.items())})


@pytest.mark.parametrize("precision,rtol", [("fp64", 1e-9), ("fp32", 1e-4)])
@pytest.mark.parametrize("physics", [Physics.PYB, Physics.PYB_GND, Physics.PYB_DRAG, Physics.PYB_GND_DRAG_DW])
@pytest.mark.parametrize("E", [128, 65])
def test_fast_spin_against_oracle(E, physics, precision, rtol):
    """E = 128: two waves of the staged kernel; E = 65: the row-store kernel with a ragged last wave"""
    rng = np.random.default_rng(1000 + E)
    env, orc = pair(E, physics, precision=precision, autoreset=False)
    f, i = random_states(rng, E, env, orc, omega=1.7)
    seed_both(env, orc, spin_mix(rng, f, orc.field_names()[0]), i)
    teacher_forced(env, orc, rng, E, rtol, active_fields(physics))
    env.close()


@pytest.mark.parametrize("physics", [Physics.PYB, Physics.PYB_GND])
def test_no_lag_generic_constants_runtime_substeps(physics):
    """link_frame_lag off (thrust axis = the current pose's, m3 = z), ctrl_freq 60: S = 4 and ring
    length 30, the generic-constant kernel with the runtime sub-step loop"""
    E = 64
    rng = np.random.default_rng(2000)
    env, orc = pair(E, physics, precision="fp64", autoreset=False, ctrl_freq=60, link_frame_lag=False)
    assert env.h.S == 4
    f, i = random_states(rng, E, env, orc, omega=1.7)
    i[orc.field_names()[1].index("step_counter")] = rng.integers(0, 200, E) * 4
    seed_both(env, orc, spin_mix(rng, f, orc.field_names()[0]), i)
    teacher_forced(env, orc, rng, E, 1e-9, active_fields(physics, lag=False))
    env.close()


def test_per_lane_clamp():
    """the world-coordinate clamp's round trip through R and R^T is committed per lane: 60 slow envs
    give the same bits whether their four wave mates are slow or spin at 250 rad/s"""
    E = 64
    rng = np.random.default_rng(3000)
    env, orc = pair(E, Physics.PYB, precision="fp64", autoreset=False)
    f, i = random_states(rng, E, env, orc, omega=1.7)
    names = orc.field_names()[0]
    w = [names.index(f"omega_{a}") for a in "xyz"]
    mates = [3, 17, 40, 63]
    acts = rng.uniform(-1, 1, (2, E, 1, 4)).astype(np.float32)

    def run(fs):
        env.set_state(torch.from_numpy(fs), torch.from_numpy(i))
        for k in range(2):
            env.step(torch.from_numpy(acts[k]))
        return env.get_state()[0].cpu().numpy()

    base = run(f.copy())
    fast = f.copy()
    fast[np.ix_(w, mates)] = 250.0 / np.sqrt(3)
    got = run(fast)
    keep = np.setdiff1d(np.arange(E), mates)
    np.testing.assert_array_equal(got[:, keep], base[:, keep])
    for e in mates:
        assert not np.array_equal(got[:, e], base[:, e])
    env.close()


def test_world_omega_round_trip():
    """state and obs keep the world frame: after one step the stored omega matches the oracle and the
    obs row's columns are its float32; the next step starts from R^T of it, which two free-running
    steps against the oracle pin"""
    E = 64
    rng = np.random.default_rng(4000)
    env, orc = pair(E, Physics.PYB, precision="fp64", autoreset=False)
    f, i = random_states(rng, E, env, orc, omega=1.7)
    names = orc.field_names()[0]
    seed_both(env, orc, spin_mix(rng, f, names), i)
    w = [names.index(f"omega_{a}") for a in "xyz"]
    active = active_fields(Physics.PYB)
    for k in range(2):
        act = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
        obs_o = orc.step(act)[0]
        obs_g = env.step(torch.from_numpy(act))[0]
        torch.cuda.synchronize()
        worst = compare_state(env, orc, 1e-9, active)
        print(f"step {k}: worst relative errors", {g: f"{v:.2e}" for g, v in sorted(worst.items())})
        fg = env.get_state()[0].cpu().numpy()
        og = obs_g.cpu().numpy()[:, 0, 9:12]
        np.testing.assert_array_equal(og, fg[w].T.astype(np.float32))
        d = np.linalg.norm(og - obs_o[:, 0, 9:12], axis=1)
        assert (d / np.maximum(np.linalg.norm(obs_o[:, 0, 9:12], axis=1), 1e-3)).max() <= 1e-4
    env.close()
