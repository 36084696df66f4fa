"""``adrp_race_roster_done`` on the device and ``RosterRolloutCollector(end_on="learners")`` (csrc/roster_kernel.h,
include/adrp_train.h, gym_pybullet_adrp_amd/rollout.py).  Needs an MI355X: -m gpu.

The kernel is compared exactly with the numpy restatement (tests/roster_end_on_reference.py) on constructed agent
states.  The collector is compared with tests/test_rollout_roster_gpu.py's loop from earlier pieces (its helpers
restated here: level0 COMPETE, a 0.3 s episode, env 1's first learner and all of env 2 put out of bounds; with two
learners also both learners of env 3, whose idle third drone stays, so that an env outlives its learners at a known
step), the reset mask taken from ``done_mask`` on the restatement's ``alive`` (tests/agents_reference.py); the same
bit equality and bars."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.envs.tracks import load_race_config  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.rollout import RosterRolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import RaceMode  # noqa: E402
from tests import agents_reference as A  # noqa: E402
from tests import ppo_reference as P  # noqa: E402
from tests import roster_reference as R  # noqa: E402
from tests.roster_end_on_reference import done_mask  # noqa: E402

L_, H_, P_, N_ = R.LEARNER, R.HARDCODED, R.POLICY, R.NONE
# (300, 3) is 300 envs: a second block with a partial last wave
SHAPES = [(1, 1, [L_]), (3, 2, [H_, L_]), (9, 8, [L_, H_, P_, N_, L_, H_, P_, L_]), (300, 3, [L_, P_, L_])]

E, N, T = 5, 3, 12
GAMMA, LAM, SEED = 0.98, 0.9, 4
EPISODE_SEC = 0.3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("E_, N_d, roles", SHAPES, ids=[f"E{s[0]}-N{s[1]}-L{sum(r == L_ for r in s[2])}" for s in SHAPES])
def test_kernel_equals_the_restatement(E_, N_d, roles):
    lib = _lib.load()
    learners = R.learners_of(roles)
    L = len(learners)
    rng = np.random.default_rng(E_ * 31 + N_d)
    io = abi.AdrpRaceRosterIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceRosterIO)
    io.num_envs, io.num_drones, io.num_learners, io.ctrl_freq = E_, N_d, L, 30.0
    for n, r in enumerate(roles):
        io.role[n] = r
        io.learner_index[n] = learners.index(n) if r == L_ else -1
    S = E_ * N_d
    state = dict(wr_gate=torch.zeros(S, dtype=torch.int32), wr_target=torch.zeros((S, 3), dtype=torch.float64),
                 wr_prev=torch.zeros((S, 3), dtype=torch.float64), alive=torch.zeros(S, dtype=torch.uint8),
                 run_return=torch.zeros(S, dtype=torch.float64), run_length=torch.zeros(S, dtype=torch.int32))
    state = {k: v.cuda() for k, v in state.items()}
    ag = abi.AdrpRaceAgentsIO()
    ag.struct_size = ctypes.sizeof(abi.AdrpRaceAgentsIO)
    ag.num_envs, ag.num_drones, ag.obs_dim, ag.num_gates = E_, N_d, 49, 4
    for k, v in state.items():
        setattr(ag, k, v.data_ptr())
    # every combination of (term, trunc, each learner alive or dead) is present: env e of round r takes combination
    # r E + e, over as many launches as that needs; the slots that are no learner's hold random bytes
    combos = [(te, tr, al) for te in (0, 1) for tr in (0, 1) for al in range(2 ** L)]
    rounds = -(-len(combos) // E_)
    seen, outputs = set(), set()
    pad = 64
    for r in range(rounds):
        term, trunc = np.zeros(E_, np.uint8), np.zeros(E_, np.uint8)
        alive = rng.integers(0, 256, (E_, N_d)).astype(np.uint8)
        for e in range(E_):
            te, tr, al = combos[(r * E_ + e) % len(combos)]
            term[e], trunc[e] = te, tr
            for l, n in enumerate(learners):
                alive[e, n] = ((al >> l) & 1) * (1 if e % 2 else 255)     # alive is "!= 0", not "== 1"
            seen.add((te, tr, al))
        want = done_mask(alive.reshape(-1), term, trunc, N_d, learners)
        state["alive"].copy_(torch.from_numpy(alive.reshape(-1)))
        term_d, trunc_d = dev(term), dev(trunc)
        # the mask inside a longer poisoned buffer: nothing before or behind its E bytes is written
        buf = torch.full((pad + E_ + pad,), 0xAB, dtype=torch.uint8, device="cuda")
        mask = buf[pad:pad + E_]
        rc = lib.adrp_race_roster_done(ctypes.byref(io), ctypes.byref(ag), term_d.data_ptr(), trunc_d.data_ptr(),
                                       mask.data_ptr(), _lib._raw_stream(0))
        assert rc == 0, lib.adrp_last_error(None).decode()
        torch.cuda.synchronize()
        got = mask.cpu().numpy()
        assert np.array_equal(got, want), r
        assert set(np.unique(got).tolist()) <= {0, 1}
        outputs |= set(got.tolist())
        assert bool((buf[:pad] == 0xAB).all()) and bool((buf[pad + E_:] == 0xAB).all())
        assert np.array_equal(state["alive"].cpu().numpy(), alive.reshape(-1))        # alive is unchanged
        assert np.array_equal(term_d.cpu().numpy(), term) and np.array_equal(trunc_d.cpu().numpy(), trunc)
    assert len(seen) == len(combos) and outputs == {0, 1}


# ---- the collector: tests/test_rollout_roster_gpu.py's setup, restated ----
def make_env(num_envs=E, **kw):
    cfg = load_race_config("level0")
    cfg["episode_len_sec"] = EPISODE_SEC
    kw = dict(dict(autoreset=False, commands=True), **kw)
    return MultiRaceAviary(cfg, num_drones=N, racemode=RaceMode.COMPETE, num_envs=num_envs, seed=9, **kw)


def make_policy(seed=3, in_dim=49, mode="relative", act_dim=4):
    w = P.make_weights(in_dim, 16, 16, act_dim, seed)
    w["action_net.weight"] = (w["action_net.weight"] * 30.0).astype(np.float32)
    return DevicePolicy(w, "tanh", 0, mode)


def plant(env, learners):
    """env 1: its first learner drone outside the bounds; env 2: every drone outside.  With two learners also env 3:
    both learners outside while its third drone stays, so that the env outlives its learners at a known step."""
    f, i = env.get_state()
    fn, _ = env.state_field_names()
    out = float(env.cfg.track.bounds_hi[0]) + 1.0
    slots = [1 * N + learners[0], 2 * N, 2 * N + 1, 2 * N + 2]
    if len(learners) > 1:
        slots += [3 * N + n for n in learners]
    for slot in slots:
        f[fn.index("pos_x"), slot] = out
    env.set_state(f, i)


def run(kind):
    """the end_on="learners" collector's rollout and the comparison loop's, whose reset mask is done_mask on the
    restatement's alive -> (col, want, things to close)"""
    pol, frozen = make_policy(), []
    if kind == "mixed":
        frozen = [make_policy(seed=5)]
        roster, roles = ["learner", "hardcoded", frozen[0]], [L_, H_, P_]
    else:
        roster, roles = ["learner", "learner", None], [L_, L_, N_]
    learners = R.learners_of(roles)
    L = len(learners)
    env = make_env()
    col = RosterRolloutCollector(env, pol, roster, T, gamma=GAMMA, gae_lambda=LAM, seed=SEED, end_on="learners")
    col.reset()
    plant(env, learners)
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
    if H_ in roles:
        cm = HardCodedCommander(obs, device=twin.device)                     # delay = drone index
        ref, offset = cm.reference_trajectory.cpu().numpy(), cm._offset.cpu().numpy()
    ro = R.Roster(E, N, roles, float(twin.CTRL_FREQ), ref, offset)
    ro.tick(None)
    ag = A.Agents(E, N, D, int(twin.cfg.track.num_gates))
    ag.reset(obs.cpu().numpy())
    plant(twin, learners)
    compact = lambda o: torch.stack([o[:, n] for n in learners]).reshape(L * E, D).contiguous()
    want = {k: [] for k in ("obs", "actions", "values", "log_probs", "starts", "valid", "rewards", "boot", "mask", "over",
                            "codes", "args", "clock")}
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
        over = (term | trunc).cpu().numpy()
        mask = done_mask(ag.alive, term.cpu().numpy(), trunc.cpu().numpy(), N, learners)
        want["over"].append(over)
        want["mask"].append(mask)
        obs, _ = twin.reset(mask=dev(mask))
        ag.reset(obs.cpu().numpy(), mask)
        ro.tick(mask)
    want["last_values"] = pol.sample(compact(obs), SEED, 0xFFFFFFFF)[2]
    want["last_dones"] = last_start
    want["stream"] = stream
    twin.close()
    return col, want, [env, pol] + frozen


@pytest.fixture(scope="module")
def mixed():
    col, want, made = run("mixed")
    yield col, want
    for x in made:
        x.close()


@pytest.fixture(scope="module")
def pair():
    col, want, made = run("pair")
    yield col, want
    for x in made:
        x.close()


def check_against_the_loop(col, want, L):
    assert (col.T, col.E, col.L, col.end_on) == (T, L * E, L, "learners") and col.valid.dtype == torch.uint8
    valid, boot, mask, over, clock = (np.stack(want[k]) for k in ("valid", "boot", "mask", "over", "clock"))
    # not vacuous (asserted on the comparison loop's side): an env is reset at a step where term | trunc is 0; a
    # bootstrap; clocks that differ between the envs
    early = (mask != 0) & (over == 0)
    assert early.sum() >= 1 and early[0, 1 if L == 1 else 3]
    assert (mask[over != 0] == 1).all() and boot.sum() >= 1 and any(len(set(c.tolist())) > 1 for c in clock)
    for name, key in (("obs", "obs"), ("actions", "actions"), ("values", "values"), ("log_probs", "log_probs")):
        assert torch.equal(bits(getattr(col, name)), bits(torch.stack(want[key]))), name
    assert np.array_equal(col.valid.cpu().numpy(), valid)
    assert np.array_equal(col.episode_starts.cpu().numpy(), np.stack(want["starts"]))
    assert np.array_equal(col.last_dones.cpu().numpy(), want["last_dones"])
    assert torch.equal(bits(col.last_values), bits(want["last_values"]))
    assert np.array_equal(col._mask.view(torch.uint8).cpu().numpy(), mask[-1])          # the last step's mask, 0 / 1 bytes
    assert len(want["stream"]) == T
    for t, (codes, args) in enumerate(want["stream"]):
        assert torch.equal(codes, dev(want["codes"][t])), f"step {t}: codes"
        assert torch.equal(args.view(torch.int64), dev(want["args"][t]).view(torch.int64)), f"step {t}: args"
    got, ref = col.rewards.cpu().numpy().astype(np.float64), np.stack(want["rewards"])
    err = np.abs(got - ref)
    print(f"worst |collector reward - loop reward| {float(err.max()):.3e}; early resets {int(early.sum())}, "
          f"valid rows {int(valid.sum())} of {valid.size}")
    assert (err <= 2.0 ** -23 * np.abs(ref) + 1e-12).all()
    assert (got[valid == 0] == 0).all()
    adv, ret = torch.zeros_like(col.rewards), torch.zeros_like(col.rewards)
    rc = _lib.load().adrp_gae(col.rewards.data_ptr(), col.values.data_ptr(), col.episode_starts.data_ptr(),
                              col.last_values.data_ptr(), col.last_dones.data_ptr(), T, L * E, GAMMA, LAM, adv.data_ptr(),
                              ret.data_ptr(), _lib._raw_stream(0))
    assert rc == 0
    assert torch.equal(bits(col.advantages), bits(adv)) and torch.equal(bits(col.returns), bits(ret))
    assert bool(torch.isfinite(col.advantages[col.valid.bool()]).all())
    return valid


def test_one_learner_every_row_is_valid(mixed):
    """learner / hardcoded / frozen policy: the env ends with its one learner, so no row waits for the opponents"""
    col, want = mixed
    valid = check_against_the_loop(col, want, 1)
    assert valid.all() and bool((col.valid == 1).all())
    # the scripted drone takes off again right after each reset of its env, the early ones included
    codes, mask = np.stack(want["codes"]), np.stack(want["mask"])
    fresh = np.concatenate([np.ones((1, E), bool), mask[:-1] != 0])
    assert np.array_equal(codes[:, :, 1] == R.CMD_TAKEOFF, fresh)


def test_two_learners_a_column_waits_only_for_its_sibling(pair):
    """learner / learner / none: a column is invalid exactly while its sibling learner is alive"""
    col, want = pair
    valid = check_against_the_loop(col, want, 2).reshape(T, 2, E)
    assert (valid == 0).sum() >= 1                              # env 1's first learner waits for the second
    assert (valid.sum(axis=1) >= 1).all()                       # never both: the env is reset with the last of them
    assert (valid[:, 1][valid[:, 0] == 0] == 1).all() and (valid[:, 0][valid[:, 1] == 0] == 1).all()


def test_end_on_env_is_the_collector_without_the_argument():
    out = []
    for kw in (dict(), dict(end_on="env")):
        pol, opp, env = make_policy(), make_policy(seed=5), make_env()
        col = RosterRolloutCollector(env, pol, ["learner", "hardcoded", opp], T, gamma=GAMMA, gae_lambda=LAM, seed=SEED, **kw)
        col.reset()
        plant(env, [0])
        col.collect()
        torch.cuda.synchronize()
        assert col.end_on == "env"
        out.append({k: getattr(col, k).clone() for k in ("obs", "actions", "rewards", "values", "log_probs", "valid",
                                                         "episode_starts", "advantages", "returns", "last_values")})
        for x in (env, pol, opp):
            x.close()
    for k in out[0]:
        a, b = out[0][k], out[1][k]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
    assert (out[0]["valid"] == 0).sum() >= 1                    # with "env" the dead learner of env 1 does wait
