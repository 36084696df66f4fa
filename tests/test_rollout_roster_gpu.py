"""RosterRolloutCollector (gym_pybullet_adrp_amd/rollout.py), PPOLearner.train on its compact columns and
PPOLearner.snapshot.  Needs an MI355X: -m gpu.

The yardstick is a loop built from the pieces that were there before the collector: ``DevicePolicy.sample`` on a
compact copy of the learner drones' rows with the same counters, ``DevicePolicy.act`` for the frozen opponent, the
numpy restatement of the roster kernels for the command rows and the clocks (tests/roster_reference.py),
``env.step((codes, args))`` on a second env of the same seed, ``get_state()``'s gate / flags rows fed to the
restatement of the agents kernels (tests/agents_reference.py), the masked ``env.reset`` and ``adrp_gae``.
Observations, actions, values, log-probabilities, validity, episode starts and every step's command rows are
compared by bit pattern; the rewards within the kernel's bar (tests/test_agents_gpu.py: 2^-23 |ref| + 1e-12); the
advantages and returns by bit pattern against ``adrp_gae`` on the collector's own rewards.

The episode length is 0.3 s, under ten env.steps: every env is truncated (with a bootstrap) and reset inside the 12-step
rollout.  Env 1's first learner drone is put outside the bounds (it is eliminated while its env goes on: rows that
are not valid), env 2's drones all are (the env terminates at once: from then on its clock differs from the others',
and its scripted drone takes off again while theirs fly their splines)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs.hover import HoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.envs.tracks import load_race_config  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.ppo import PPOLearner  # noqa: E402
from gym_pybullet_adrp_amd.rollout import RosterRolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import RaceMode  # noqa: E402
from tests import agents_reference as A  # noqa: E402
from tests import ppo_reference as P  # noqa: E402
from tests import roster_reference as R  # noqa: E402

E, N, T = 5, 3, 12
GAMMA, LAM, SEED = 0.98, 0.9, 4
EPISODE_SEC = 0.3


def make_env(num_envs=E, **kw):
    cfg = load_race_config("level0")
    cfg["episode_len_sec"] = EPISODE_SEC
    kw = dict(dict(autoreset=False, commands=True), **kw)
    return MultiRaceAviary(cfg, num_drones=N, racemode=RaceMode.COMPETE, num_envs=num_envs, seed=9, **kw)


def make_policy(seed=3, in_dim=49, mode="relative", act_dim=4):
    w = P.make_weights(in_dim, 16, 16, act_dim, seed)
    w["action_net.weight"] = (w["action_net.weight"] * 30.0).astype(np.float32)
    return DevicePolicy(w, "tanh", 0, mode)


def plant(env, learner):
    """env 1: its first learner drone outside the bounds; env 2: every drone outside"""
    f, i = env.get_state()
    fn, _ = env.state_field_names()
    out = float(env.cfg.track.bounds_hi[0]) + 1.0
    for slot in (1 * N + learner, 2 * N, 2 * N + 1, 2 * N + 2):
        f[fn.index("pos_x"), slot] = out
    env.set_state(f, i)


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(kind):
    """the collector's rollout and the comparison loop's -> (col, learner policy, want, frozen policies)"""
    pol, frozen = make_policy(), []
    if kind == "mixed":
        frozen = [make_policy(seed=5)]
        roster, roles = ["learner", "hardcoded", frozen[0]], [R.LEARNER, R.HARDCODED, R.POLICY]
    else:
        roster, roles = ["learner", "learner", None], [R.LEARNER, R.LEARNER, R.NONE]
    learners = R.learners_of(roles)
    L = len(learners)
    env = make_env()
    col = RosterRolloutCollector(env, pol, roster, T, gamma=GAMMA, gae_lambda=LAM, seed=SEED)
    col.reset()
    plant(env, learners[0])
    stream, env_step = [], env.step
    env.step = lambda cmd: (stream.append((cmd[0].clone(), cmd[1].clone())), env_step(cmd))[1]
    col.collect()
    torch.cuda.synchronize()

    twin = make_env()
    D = twin.h.D
    inames = twin.state_field_names()[1]
    gi, fi = inames.index("gate"), inames.index("flags")
    obs, _ = twin.reset()
    ref = offset = None
    if R.HARDCODED in roles:
        cm = HardCodedCommander(obs, device=twin.device)                     # delay = drone index
        ref, offset = cm.reference_trajectory.cpu().numpy(), cm._offset.cpu().numpy()
    ro = R.Roster(E, N, roles, float(twin.CTRL_FREQ), ref, offset)
    ro.tick(None)
    ag = A.Agents(E, N, D, int(twin.cfg.track.num_gates))
    ag.reset(obs.cpu().numpy())
    plant(twin, learners[0])
    compact = lambda o: torch.stack([o[:, n] for n in learners]).reshape(L * E, D).contiguous()
    want = {k: [] for k in ("obs", "actions", "values", "log_probs", "starts", "valid", "rewards", "boot", "mask", "codes",
                            "args", "clock")}
    last_start = np.ones(L * E, np.float32)
    for t in range(T):
        rows = compact(obs)
        ea, a, v, lp = pol.sample(rows, SEED, t)
        want["obs"].append(rows)
        want["starts"].append(last_start)
        want["actions"].append(a)
        want["values"].append(v)
        want["log_probs"].append(lp)
        sp = np.zeros((N, E, 4), np.float32)
        for n, c in enumerate(roster):
            if isinstance(c, DevicePolicy):
                sp[n] = c.act(obs[:, n].contiguous()).cpu().numpy()
        want["clock"].append(ro.clock.copy())
        codes, args = ro.act(sp, ea.view(L, E, 4).cpu().numpy())
        want["codes"].append(codes)
        want["args"].append(args)
        obs, _, term, trunc, _ = twin.step((dev(codes), dev(args)))
        tv = pol.sample(compact(obs), SEED, 0xFFFFFFFF)[2]
        _, i = twin.get_state()
        o = R.compact_step(ag, learners, obs.cpu().numpy(), i[gi].cpu().numpy(), i[fi].cpu().numpy(), term.cpu().numpy(),
                           trunc.cpu().numpy(), tv.cpu().numpy(), GAMMA)
        want["valid"].append(o["valid"])
        want["rewards"].append(o["stored"])
        want["boot"].append(o["boot"])
        last_start = o["next_start"]
        mask = (term | trunc).cpu().numpy()
        want["mask"].append(mask)
        obs, _ = twin.reset(mask=term | trunc)
        ag.reset(obs.cpu().numpy(), mask)
        ro.tick(mask)
    want["last_values"] = pol.sample(compact(obs), SEED, 0xFFFFFFFF)[2]
    want["last_dones"] = last_start
    want["stream"] = stream
    twin.close()
    return col, pol, want, frozen, env


def close_all(col, pol, frozen, env):
    env.close()
    for p in [pol] + frozen:
        p.close()


@pytest.fixture(scope="module")
def mixed():
    col, pol, want, frozen, env = run("mixed")
    yield col, pol, want
    close_all(col, pol, frozen, env)


@pytest.fixture(scope="module")
def pair():
    col, pol, want, frozen, env = run("pair")
    yield col, pol, want
    close_all(col, pol, frozen, env)


def check_against_the_loop(col, want, L):
    assert (col.T, col.E, col.L) == (T, L * E, L) and col.valid.dtype == torch.uint8
    assert tuple(col.obs.shape[:2]) == (T, L * E) and tuple(col.rewards.shape) == (T, L * E)
    # not vacuous (asserted on the comparison loop's side): an env reset inside the rollout, a learner column with a
    # row that is not valid, a bootstrap, clocks that differ between the envs
    valid, boot, mask, clock = (np.stack(want[k]) for k in ("valid", "boot", "mask", "clock"))
    assert mask[:-1].sum() >= 1 and (valid == 0).sum() >= 1 and boot.sum() >= 1
    assert mask[0, 2] and not valid[1:7, 1].any() and any(len(set(c.tolist())) > 1 for c in clock)
    for name, key in (("obs", "obs"), ("actions", "actions"), ("values", "values"), ("log_probs", "log_probs")):
        assert torch.equal(bits(getattr(col, name)), bits(torch.stack(want[key]))), name
    assert np.array_equal(col.valid.cpu().numpy(), valid)
    assert np.array_equal(col.episode_starts.cpu().numpy(), np.stack(want["starts"]))
    assert np.array_equal(col.last_dones.cpu().numpy(), want["last_dones"])
    assert torch.equal(bits(col.last_values), bits(want["last_values"]))
    # the command stream of every step
    assert len(want["stream"]) == T
    for t, (codes, args) in enumerate(want["stream"]):
        assert torch.equal(codes, dev(want["codes"][t])), f"step {t}: codes"
        assert torch.equal(args.view(torch.int64), dev(want["args"][t]).view(torch.int64)), f"step {t}: args"
    got, ref = col.rewards.cpu().numpy().astype(np.float64), np.stack(want["rewards"])
    err = np.abs(got - ref)
    print(f"worst |collector reward - loop reward| {float(err.max()):.3e}")
    assert (err <= 2.0 ** -23 * np.abs(ref) + 1e-12).all()
    assert (got[valid == 0] == 0).all()
    # advantages and returns: adrp_gae over the L E columns of the collector's own rewards
    adv, ret = torch.zeros_like(col.rewards), torch.zeros_like(col.rewards)
    rc = _lib.load().adrp_gae(col.rewards.data_ptr(), col.values.data_ptr(), col.episode_starts.data_ptr(),
                              col.last_values.data_ptr(), col.last_dones.data_ptr(), T, L * E, GAMMA, LAM, adv.data_ptr(),
                              ret.data_ptr(), _lib._raw_stream(0))
    assert rc == 0
    assert torch.equal(bits(col.advantages), bits(adv)) and torch.equal(bits(col.returns), bits(ret))
    assert bool(torch.isfinite(col.advantages[col.valid.bool()]).all())
    s = col.episode_summary()
    ended = col.ep_length.cpu().numpy() > 0
    assert s["episodes"] == int(ended.sum()) >= L * E
    assert s["ep_rew_mean"] == pytest.approx(float(col.ep_return.cpu().numpy()[ended].mean()), rel=1e-12)
    assert s["ep_len_mean"] == pytest.approx(float(col.ep_length.cpu().numpy()[ended].mean()), rel=1e-12)


def test_collector_equals_the_loop_from_earlier_pieces(mixed):
    """learner / hardcoded / frozen policy"""
    col, pol, want = mixed
    check_against_the_loop(col, want, 1)
    codes = np.stack(want["codes"])
    # the scripted drone takes off at every env's first step and again right after each reset of its env, and flies
    # its spline in between; the learner and the frozen policy always send FULLSTATE
    mask = np.stack(want["mask"])
    fresh = np.concatenate([np.ones((1, E), bool), mask[:-1] != 0])
    assert np.array_equal(codes[:, :, 1] == R.CMD_TAKEOFF, fresh) and (codes[:, :, 1][~fresh] == R.CMD_FULLSTATE).all()
    assert fresh[1, 2] and not fresh[1, 0] and fresh[2:, [0, 1, 3, 4]].any()
    assert (codes[:, :, [0, 2]] == R.CMD_FULLSTATE).all()


def test_two_learners_are_drone_major_columns(pair):
    """learner / learner / none: column l E + e is learner l in env e"""
    col, pol, want = pair
    check_against_the_loop(col, want, 2)
    assert (np.stack(want["codes"])[:, :, 2] == R.CMD_NONE).all()
    # the columns against the env's own rows: after the rollout the env holds the observation last_values was taken on
    obs = col._env_obs
    for l, n in enumerate((0, 1)):
        assert torch.equal(col._post.view(2, E, -1)[l], obs[:, n])
    # the two learners saw different rows and drew different Philox rows
    assert not torch.equal(col.obs[0, :E], col.obs[0, E:]) and not torch.equal(col.actions[0, :E], col.actions[0, E:])


def test_train_and_snapshot(pair):
    """train(col) with fixed permutations [n_epochs, n_valid] against manual update calls over the same slices:
    parameters, m and v torch.equal.  snapshot(): the learner policy's deterministic output before the update, and
    still that after it, while the learner's own output has moved."""
    col, pol, _ = pair
    n_epochs, batch = 2, 32
    n = col.T * col.E
    valid = col.valid.view(n).bool()
    rows = torch.nonzero(valid).view(-1)
    nv = rows.numel()
    assert 0 < nv < n
    g = torch.Generator().manual_seed(1)
    perms = torch.stack([rows[torch.randperm(nv, generator=g).cuda()] for _ in range(n_epochs)])
    made = []

    def fresh():
        made.append(make_policy())
        made.append(PPOLearner(made[-1], n_epochs=n_epochs, batch_size=batch, seed=0))
        return made[-1]

    a = fresh()
    x = col.obs[0].contiguous()
    before = a.policy.act(x).clone()
    snap = a.snapshot()
    made.insert(0, snap)
    assert isinstance(snap, DevicePolicy) and not snap.has_critic and snap.h.value != a.policy.h.value
    assert (snap.mode, snap.activation, snap.in_dim, snap.act_dim) == (a.policy.mode, "tanh", 49, 4)
    assert torch.equal(bits(snap.act(x)), bits(before))
    other = a.snapshot(mode="absolute")
    made.insert(0, other)
    assert other.mode != snap.mode and not torch.equal(other.act(x), before)
    stats = a.train(col, permutations=perms)
    assert stats.shape == (n_epochs, (nv + batch - 1) // batch, 5)
    assert torch.equal(bits(snap.act(x)), bits(before))                   # the snapshot did not move
    assert not torch.equal(a.policy.act(x), before)                       # the learner did
    got = (a.state_dict(), a.optimizer_state_dict())
    b = fresh()
    flat = (col.obs.view(n, -1), col.actions.view(n, -1), col.values.view(n), col.log_probs.view(n),
            col.advantages.view(n), col.returns.view(n))
    for e in range(n_epochs):
        for s in range(0, nv, batch):
            b.update(*flat, perms[e, s:s + batch].contiguous())
    want = (b.state_dict(), b.optimizer_state_dict())
    for k in got[0]:
        assert torch.equal(got[0][k], want[0][k]), k
        assert torch.equal(got[1]["exp_avg"][k], want[1]["exp_avg"][k]), k
        assert torch.equal(got[1]["exp_avg_sq"][k], want[1]["exp_avg_sq"][k]), k
    assert got[1]["step"] == want[1]["step"] == n_epochs * ((nv + batch - 1) // batch)
    for obj in reversed(made):               # learners before their policies
        obj.close()


def test_refusals():
    pol = make_policy()
    env = make_env(2)
    roster = ["learner", "hardcoded", None]
    hover = HoverAviary(num_envs=2)
    with pytest.raises(ValueError, match="MultiRaceAviary"):
        RosterRolloutCollector(hover, pol, roster, 4)
    auto = make_env(2, autoreset=True)
    with pytest.raises(ValueError, match="autoreset=False"):
        RosterRolloutCollector(auto, pol, roster, 4)
    setpoint = make_env(2, commands=False)
    with pytest.raises(ValueError, match="commands=True"):
        RosterRolloutCollector(setpoint, pol, roster, 4)
    with pytest.raises(ValueError, match="no 'learner' drone"):
        RosterRolloutCollector(env, pol, ["hardcoded", None, pol], 4)
    with pytest.raises(ValueError, match="2 entries for 3 drones"):
        RosterRolloutCollector(env, pol, ["learner", "hardcoded"], 4)
    raw, narrow, wide = make_policy(mode="raw"), make_policy(mode="raw", act_dim=3), make_policy(in_dim=80)
    for bad in (raw, narrow):
        with pytest.raises(ValueError, match="drone 2: a race policy emits a setpoint"):
            RosterRolloutCollector(env, pol, ["learner", None, bad], 4)
    with pytest.raises(ValueError, match="drone 1: the policy reads 80 inputs"):
        RosterRolloutCollector(env, pol, ["learner", wide, None], 4)
    with pytest.raises(ValueError, match="not a roster entry"):
        RosterRolloutCollector(env, pol, ["learner", "scripted", None], 4)
    with pytest.raises(ValueError, match="planner must be"):
        RosterRolloutCollector(env, pol, roster, 4, planner="gpu")
    col = RosterRolloutCollector(env, pol, roster, 4)
    with pytest.raises(RuntimeError, match="reset\\(\\) first"):
        col.collect()
    for x in (env, auto, setpoint, hover, pol, raw, narrow, wide):
        x.close()
