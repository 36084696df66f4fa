"""evaluate_policy, the collector's Monitor window and the Evaluator on the device
(gym_pybullet_adrp_amd/evaluation.py, rollout.py) against host loops that feed the numpy restatement of
SB3's accounts (tests/episode_reference.py).  Needs an MI355X: -m gpu.

Both arms launch the same policy and step kernels on the same inputs (a second env of the same seed), so
the episode returns (float64 sums of the float32 step rewards, in step order) and lengths must be equal
exactly: any difference is an accounting error.  An env carries history into its next evaluation (reset()
goes on in the env's random streams; a HoverAviary re-keyed with reset(seed=...) still gave other episodes
than a new one), so every arm of every comparison runs on an env of its own, fresh from the same
constructor call."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.evaluation import EpisodeStats, Evaluator, episode_count_targets, evaluate_policy  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from tests import episode_reference as R  # noqa: E402
from tests import ppo_reference as P  # noqa: E402


def random_policy(in_dim, act_dim, seed, mode="raw", gain=1.0, hidden=16):
    """fixed-seed actor + critic; ``gain`` scales action_net so the clipped actions leave the hover band"""
    w = P.make_weights(in_dim, hidden, hidden, act_dim, seed)
    w["action_net.weight"] = (w["action_net.weight"] * gain).astype(np.float32)
    w["action_net.bias"] = (w["action_net.bias"] * gain).astype(np.float32)
    return DevicePolicy(w, "tanh", 0, mode)


def host_loop(policy, env, n_eval_episodes, deterministic=True, seed=0, joint=False):
    """SB3's evaluate_policy with a host read every step: the reference accounts fed the env's outputs"""
    E = env.num_envs
    obs, _ = env.reset()
    width = policy.act_dim if policy.mode == 0 else 4
    act = torch.empty(tuple(env._act_shape) if joint else obs.shape[:-1] + (width,), dtype=torch.float32, device=obs.device)
    rows = E if joint else obs.shape[0] * obs.shape[1]

    def step_fn(t):
        x = obs.view(E, -1) if joint else obs
        if deterministic:
            policy.act(x, out=act)
        else:
            policy.sample(x, seed, t, env_act=act.view(rows, -1))
        _, rew, term, trunc, _ = env.step(act)
        return rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy()
    return R.evaluate_policy_accounts(step_fn, E, n_eval_episodes)


@pytest.fixture(scope="module")
def hover():
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.utils.enums import ActionType
    envs = []

    def make():
        envs.append(HoverAviary(act=ActionType.RPM, num_envs=5, seed=3, init_noise={"rpy": 0.2}))
        return envs[-1]
    pol = random_policy(make().h.D, 4, 21, gain=60.0)
    want = host_loop(pol, make(), 7)
    yield make, pol, want
    pol.close()
    for e in envs:
        e.close()


def test_hover_equals_the_host_loop(hover):
    make, pol, (want_r, want_n, steps) = hover
    got_r, got_n = evaluate_policy(pol, make(), n_eval_episodes=7, return_episode_rewards=True)
    print("hover returns", got_r, "lengths", got_n, "host steps", steps)
    assert len(set(want_n)) >= 2                  # some episodes truncate early (tilt), not all at one length
    assert len(got_r) == 7 and got_r == want_r and got_n == want_n
    mean, std = evaluate_policy(pol, make(), n_eval_episodes=7)
    assert (mean, std) == (float(np.mean(want_r)), float(np.std(want_r)))


@pytest.mark.parametrize("poll_every", [1, 7])
def test_hover_result_does_not_depend_on_polling(hover, poll_every):
    make, pol, (want_r, want_n, _) = hover
    got = evaluate_policy(pol, make(), n_eval_episodes=7, return_episode_rewards=True, poll_every=poll_every)
    assert got == (want_r, want_n)


def test_hover_stochastic_equals_the_host_loop(hover):
    make, pol, (det_r, _, _) = hover
    want_r, want_n, _ = host_loop(pol, make(), 7, deterministic=False, seed=5)
    got = evaluate_policy(pol, make(), n_eval_episodes=7, deterministic=False, return_episode_rewards=True, seed=5)
    assert got == (want_r, want_n)
    assert want_r != det_r                        # the sampled actions are other actions


def test_max_steps(hover):
    make, pol, (_, want_n, steps) = hover
    with pytest.raises(RuntimeError, match="still open"):
        evaluate_policy(pol, make(), n_eval_episodes=7, max_steps=steps - 1, poll_every=3)
    assert len(evaluate_policy(pol, make(), n_eval_episodes=7, max_steps=steps, return_episode_rewards=True)[0]) == 7


def test_multihover_joint_policy():
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    make = lambda: MultiHoverAviary(num_drones=2, num_envs=3, seed=5, init_noise={"rpy": 0.2})
    a, b = make(), make()
    pol = random_policy(144, 8, 22, gain=60.0)
    assert a.h.D * 2 == 144 and a.h.A * 2 == 8
    want_r, want_n, _ = host_loop(pol, b, 4, joint=True)
    got = evaluate_policy(pol, a, n_eval_episodes=4, return_episode_rewards=True)
    print("multihover returns", got[0], "lengths", got[1])
    assert got == (want_r, want_n) and len(want_r) == 4
    pol.close(); a.close(); b.close()


def test_one_drone_race_relative_mode():
    from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary
    make = lambda: MultiRaceAviary("level0", num_drones=1, num_envs=4, seed=3, reward="wrapper")
    a, b, c = make(), make(), make()
    pol = random_policy(49, 4, 23, mode="relative", gain=30.0)
    want_r, want_n, steps = host_loop(pol, b, 6)
    got_r, got_n = evaluate_policy(pol, a, n_eval_episodes=6, return_episode_rewards=True)
    print("race returns", got_r, "lengths", got_n)
    assert (got_r, got_n) == (want_r, want_n)
    limit = int(a.cfg.track.episode_len_sec * a.CTRL_FREQ) + 2
    assert all(1 <= n <= limit for n in got_n)
    # episode_times: the same episodes through an EpisodeStats of our own on a third env
    st = EpisodeStats(4, 0, capacity=6, ring=False, quota=episode_count_targets(6, 4))
    obs, _ = c.reset()
    act = torch.empty((4, 1, 4), device="cuda")
    for _ in range(steps):
        pol.act(obs, out=act)
        obs, rew, term, trunc, _ = c.step(act)
        st.step(rew, term, trunc)
    assert st.remaining() == 0 and st.episodes()[1].tolist() == got_n
    assert st.episode_times(c.CTRL_FREQ).tolist() == [(n - 1) / c.CTRL_FREQ for n in got_n]
    pol.close(); a.close(); b.close(); c.close()


def test_refusals():
    from gym_pybullet_adrp_amd.envs.ctrl import CtrlAviary
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary
    pol = random_policy(49, 4, 24, mode="relative")
    for env, word in ((CtrlAviary(num_envs=2), "never ends an episode"),
                      (HoverAviary(num_envs=2, autoreset=False), "autoreset"),
                      (MultiRaceAviary("level0", num_drones=2, num_envs=2), "per-drone agents of a multi-drone race are not evaluated")):
        with pytest.raises(ValueError, match=word):
            evaluate_policy(pol, env, n_eval_episodes=2)
        with pytest.raises(ValueError, match=word):
            Evaluator(env, pol)
        env.close()
    pol.close()


def collector_setup(with_stats, n_steps=300):
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.rollout import RolloutCollector
    from gym_pybullet_adrp_amd.utils.enums import ActionType
    env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=8, seed=4, initial_xyzs=[0, 0, 1.0],
                      init_noise={"rpy": 0.35, "omega": 2.0, "vel": 0.5})
    pol = random_policy(env.h.D, 1, 25, gain=20.0)
    st = EpisodeStats(8, 0, capacity=100, ring=True) if with_stats else None
    col = RolloutCollector(env, pol, n_steps, seed=2, episode_stats=st)
    return env, pol, st, col


def test_collector_window():
    """8 envs x 300 steps: ep_rew_mean / ep_len_mean are the reference window's over the env's own rewards
    (read from env._rew each step of a second identical run, not from col.rewards, which carry the time-limit
    bootstrap), and the hook changes nothing the collector stores"""
    env, pol, st, col = collector_setup(True)
    col.reset()
    col.collect()
    env2, pol2, _, col2 = collector_setup(False)
    ref = R.Accounts(8, 100, True)
    step = env2.step

    def recording_step(a):
        out = step(a)
        ref.step(out[1].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy())
        return out
    env2.step = recording_step
    col2.reset()
    col2.collect()
    torch.cuda.synchronize()
    for k in ("obs", "rewards", "advantages", "actions", "values"):
        assert torch.equal(getattr(col, k), getattr(col2, k)), k
    assert ref.total >= 8                                  # every env ends at least once in 300 > 241 steps
    boots = (col._trunc & ~col._term).sum().item()
    assert boots > 0                                       # the stored rewards do carry bootstraps
    got, want = st.summary(), ref.summary()
    print("collector window", got)
    assert got["total"] == ref.total and got["n"] == min(ref.total, 100)
    r, n, e = st.episodes()
    rr, rn, re = ref.episodes()
    assert np.array_equal(r, rr) and np.array_equal(n, rn) and np.array_equal(e, re)
    k, u = len(rr), 2.0 ** -52
    assert abs(got["ep_rew_mean"] - want["ep_rew_mean"]) <= k * u * np.abs(rr).max()
    assert abs(got["ep_len_mean"] - want["ep_len_mean"]) <= k * u * rn.max()
    for x in (pol, pol2, env, env2):
        x.close()


def test_collect_is_capturable_with_the_hook():
    env, pol, st, col = collector_setup(True, n_steps=12)
    col.reset()
    col.collect()                                          # eager warm-up
    torch.cuda.synchronize()
    before = int(st.meta[2])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        col.collect()
    assert int(st.meta[2]) == before                       # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert int(st.meta[2]) == before + 12
    pol.close(); env.close()


def test_evaluator_on_the_device(tmp_path):
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.ppo import PPOLearner
    from gym_pybullet_adrp_amd.utils.enums import ActionType
    env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=3, seed=1, init_noise={"rpy": 0.3})
    pol = random_policy(env.h.D, 1, 26, gain=20.0)
    learner = PPOLearner(pol)
    best, logs = str(tmp_path / "best.pth"), str(tmp_path / "logs")
    ev = Evaluator(env, pol, n_eval_episodes=4, eval_freq=100, best_path=best, log_path=logs)
    assert ev.on_rollout(64 * 8, 64, learner) is True and ev.n_evaluations == 0
    assert ev.on_rollout(128 * 8, 128, learner) is True and ev.n_evaluations == 1
    assert ev.on_rollout(256 * 8, 256, learner) is True and ev.n_evaluations == 2
    z = np.load(os.path.join(logs, "evaluations.npz"))
    assert z["results"].shape == (2, 4) and z["ep_lengths"].shape == (2, 4) and z["timesteps"].tolist() == [1024, 2048]
    assert ev.best_mean_reward == float(z["results"].mean(1).max())
    assert ev.evaluations_length == z["ep_lengths"].tolist()
    sd = torch.load(best)
    assert set(sd) == set(P.KEYS) and all(not v.is_cuda for v in sd.values())
    pol2 = DevicePolicy({k: v.numpy() for k, v in sd.items()}, "tanh", 0, "raw")
    x = torch.randn(5, env.h.D, device="cuda")
    assert torch.equal(pol2.act(x), pol.act(x))
    learner.close(); pol2.close(); pol.close(); env.close()
