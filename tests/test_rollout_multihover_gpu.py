"""On-device PPO rollout collection (gym_pybullet_adrp_amd/rollout.py) through the wide policy kernels:
MultiHoverAviary as the one joint agent SB3's MlpPolicy makes of it (N D inputs, N A outputs) and
HoverAviary at its default RPM action type (72 -> 4), against the float64 restatement of SB3 2.3.2's
ActorCriticPolicy.forward / RolloutBuffer.compute_returns_and_advantage (oracle/policy.py).
Needs an MI355X: -m gpu.

Bars, as the narrow collector tests (tests/test_rollout_gpu.py): stored action and value 5e-5 (value
relative to max(1, |v|)), log-prob 1e-4 relative, GAE bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.policy import DevicePolicy, rollout  # noqa: E402
from gym_pybullet_adrp_amd.rollout import RolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import ActionType  # noqa: E402
from oracle import policy as OP  # noqa: E402
from tests.test_policy_wide import actor, critic, random_net  # noqa: E402
from tests.test_policy_wide_gpu import wide_eps  # noqa: E402

E = 256
NOISE = {"xyz": 0.1, "rpy": 0.3, "vel": 0.3, "omega": 1.0}


def check_collector(env, N, A, D, T, steps, seed=7):
    """two collect() calls of a random in -> 64 -> 64 -> N A actor / critic on env; the second rollout's
    buffer is checked"""
    wd = random_net(np.random.default_rng(N * D + A), N * D, 64, 64, N * A)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    col = RolloutCollector(env, pol, T, seed=seed)
    col.reset()
    col.collect()
    col.collect()
    torch.cuda.synchronize()
    obs, actions = col.obs.cpu().numpy(), col.actions.cpu().numpy()
    assert obs.shape == (T, E, N * D) and actions.shape == (T, E, N * A)
    assert col.rewards.shape == (T, E) and col.values.shape == (T, E)
    w, v = actor(wd), critic(wd)
    for t in steps:
        e_ref = wide_eps(E, seed, T + t, N * A)             # second rollout: counter = rollout * T + t
        a_ref, v_ref, lp_ref = OP.sample(w, v, obs[t], False, e_ref)
        ea = np.abs(actions[t] - a_ref).max()
        ev = np.abs(col.values[t].cpu().numpy() - v_ref).max()
        el = np.abs(col.log_probs[t].cpu().numpy() - lp_ref).max()
        print(f"N={N} A={A} t={t}: action {ea:.3e} value {ev:.3e} log_prob {el:.3e}")
        assert ea <= 5e-5
        assert ev <= 5e-5 * max(1, np.abs(v_ref).max())
        assert el <= 1e-4 * max(1, np.abs(lp_ref).max())
    a_ref, r_ref = OP.gae(col.rewards.cpu().numpy(), col.values.cpu().numpy(), col.episode_starts.cpu().numpy(),
                          col.last_values.cpu().numpy(), col.last_dones.cpu().numpy(), 0.99, 0.95)
    np.testing.assert_array_equal(col.advantages.cpu().numpy(), a_ref)
    np.testing.assert_array_equal(col.returns.cpu().numpy(), r_ref)
    # the joint action reaches the drones row-major [n][a]: where no reset intervened, the newest slot of
    # drone n's action history in obs[t + 1] (the last A floats of its row) is clip(actions[t])[n A : (n + 1) A]
    starts = col.episode_starts.cpu().numpy()
    cont = 0
    for t in range(T - 1):
        keep = starts[t + 1] == 0
        cont += int(keep.sum())
        newest = obs[t + 1].reshape(E, N, D)[keep][:, :, D - A:].reshape(-1, N * A)
        np.testing.assert_array_equal(newest, np.clip(actions[t][keep], -1, 1))
    assert cont > E
    assert starts.sum() > 0                                 # auto-resets inside the rollout
    pol.close()
    env.close()


def test_collect_multihover_joint_agent():
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    env = MultiHoverAviary(num_drones=2, act=ActionType.RPM, num_envs=E, seed=4, init_noise=NOISE)
    check_collector(env, 2, 4, 72, 16, (0, 5, 15))


def test_collect_multihover_three_drones_one_d_rpm():
    """81 -> 3: rows of 27 floats (no float4 staging), a lane group of 4 with an inactive lane"""
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    env = MultiHoverAviary(num_drones=3, act=ActionType.ONE_D_RPM, num_envs=E, seed=4, init_noise=NOISE)
    check_collector(env, 3, 1, 27, 8, (0, 5, 7))


def test_collect_hover_rpm():
    """learn.py's default single-agent task: HoverAviary(act=RPM), 72 -> 4"""
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    env = HoverAviary(act=ActionType.RPM, num_envs=E, seed=4, initial_xyzs=[0, 0, 1.0], init_noise=NOISE)
    check_collector(env, 1, 4, 72, 8, (0, 5, 7))


def test_joint_rollout_helper_and_refusals():
    """rollout(): a policy as wide as the joint row drives MultiHoverAviary through [E, N A] -> [E, N, A];
    the collector refuses a multi-drone race (per-drone agents) and a policy that is not the joint width"""
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary
    env = MultiHoverAviary(num_drones=2, num_envs=64, seed=1)
    wd = random_net(np.random.default_rng(0), 144, 64, 64, 8)
    pol = DevicePolicy(wd, "tanh", 0, "raw")
    env.reset()
    act = torch.empty((64, 2, 4), device=env.device)
    out = rollout(env, pol, 3, act)
    torch.cuda.synchronize()
    assert out[0].shape == (64, 2, 72) and torch.isfinite(out[0]).all()
    # the newest action-history slot of each drone is the action rollout() fed the last step (an env that
    # the step reset has a cleared history)
    keep = ~(out[2] | out[3]).cpu().numpy()
    assert keep.sum() > 32
    np.testing.assert_array_equal(out[0][:, :, 68:].cpu().numpy()[keep], act.cpu().numpy()[keep])
    per_drone = DevicePolicy(random_net(np.random.default_rng(0), 72, 64, 64, 4), "tanh", 0, "raw")
    with pytest.raises(ValueError, match="joint"):
        RolloutCollector(env, per_drone, 4)
    race = MultiRaceAviary("level0", num_drones=2, num_envs=64, seed=1)
    with pytest.raises(ValueError, match="MultiHoverAviary"):
        RolloutCollector(race, per_drone, 4)
    for x in (env, race, pol, per_drone):
        x.close()
