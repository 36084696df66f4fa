"""The batched race evaluation on the device (csrc/sim_kernel.h, gym_pybullet_adrp_amd/sim.py).  Needs an
MI355X: -m gpu.

The yardsticks are the pieces the package already has: ``HardCodedCommander.predict`` (the torch path of the
scripted controller, itself pinned by tests/golden/hardcoded_golden.npz), ``DevicePolicy.act`` on a contiguous copy
of a drone's rows, and the numpy restatement of the results accounting (tests/sim_reference.py, pinned by hand in
tests/test_sim_abi.py).  Everything the two kernels do is selects, copies, one table read, one float64 multiply
and truncation and a float64 running sum in step order, so every comparison is exact: ``torch.equal`` /
``np.array_equal`` (bit patterns for the float64 returns).  The one bound is the golden stream's own, 1e-12
absolute, the bound tests/test_hardcoded.py applies to the torch path."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.commands import CMD_ARGS, COMMAND_CODE  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.sim import ControllerBank, RaceResults, simulate  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Command  # noqa: E402
from tests import ppo_reference as P  # noqa: E402
from tests import sim_reference as R  # noqa: E402

CODES = {c: COMMAND_CODE[c] for c in (Command.NONE, Command.FULLSTATE, Command.TAKEOFF, Command.NOTIFY, Command.LAND)}
DEVICE_BUFFERS = ("open", "run_return", "run_length", "run_gates", "run_finish", "run_elim", "meta", "log_return",
                  "log_length", "log_term", "log_trunc", "log_gates", "log_finish", "log_elim")


def reset_obs(config, E, N):
    env = MultiRaceAviary(config, num_drones=N, num_envs=E, seed=5, autoreset=False)
    obs = env.reset()[0].clone()
    env.close()
    return obs


def stub_env(E, N, D):
    """what ControllerBank reads of an env: the shape and the device"""
    return types.SimpleNamespace(num_envs=E, NUM_DRONES=N, device=torch.device("cuda", 0), h=types.SimpleNamespace(D=D))


def random_policy(seed, mode="relative", hidden=16, in_dim=49):
    w = P.make_weights(in_dim, hidden, hidden, 4, seed)
    w["action_net.weight"] = (w["action_net.weight"] * 30.0).astype(np.float32)      # some outputs reach the clip
    return DevicePolicy(w, "tanh", 0, mode)


# ---- controller kernel, scripted drones -----------------------------------------------------------------------

@pytest.mark.parametrize("config, freq", [("level0", 25), ("getting_started", 30)])
@pytest.mark.parametrize("E, N", [(1, 1), (3, 2), (70, 3)])
def test_scripted_drones_equal_the_torch_commander(config, freq, E, N):
    """every step of the whole flight (TAKEOFF, every FULLSTATE sample, NOTIFY, LAND, NONE) of every drone, delays
    arange(N); (70, 3) is 210 lanes: past one wave of 64, with a partial last wave"""
    obs = reset_obs(config, E, N)
    bank = ControllerBank(stub_env(E, N, obs.shape[2]), "hardcoded")
    bank.reset(obs)
    hc = HardCodedCommander(obs)                       # a second, independent commander
    assert torch.equal(bank.commander.reference_trajectory, hc.reference_trajectory)
    seen = torch.zeros((11, N), dtype=torch.bool, device=obs.device)
    for k in range((2 + N + 12 + 1) * freq + 1):
        t = k / freq
        codes, args = bank.predict(obs, t)
        want_c, want_a = hc.predict(t)
        assert codes.dtype == torch.int32 and args.dtype == torch.float64 and args.shape == (E, N, CMD_ARGS)
        assert torch.equal(codes, want_c), f"step {k}: codes"
        assert torch.equal(args, want_a), f"step {k}: args"
        seen[codes[0].long(), torch.arange(N, device=obs.device)] = True
    assert torch.equal(bank.phase.bool(), hc._flags) and bool(hc._flags.all())
    for c in CODES.values():
        assert bool(seen[c].all()), f"command {c} never sent"


def test_scripted_drones_reproduce_the_golden_stream():
    """the reference controller's own command stream (tests/golden/hardcoded_golden.npz) through the kernel path,
    under the bounds tests/test_hardcoded.py applies to the torch path"""
    from tests.test_hardcoded import G, K, fixture_commands
    E = 3
    # (the fixture's float64 observation as it is: the reference plans from float64)
    obs0 = torch.from_numpy(np.broadcast_to(G["hc_obs0"], (E, 2, G["hc_obs0"].shape[1])).copy()).cuda()
    bank = ControllerBank(stub_env(E, 2, obs0.shape[2]), ["hardcoded", "hardcoded"])
    bank.reset(obs0)
    np.testing.assert_allclose(bank.commander.reference_trajectory[0].cpu().numpy(), G["hc_ref"], rtol=0, atol=1e-12)
    f = float(G["hc_ctrl_freq"])
    got_c, got_a = [], []
    for k in range(K):
        codes, args = bank.predict(obs0, k / f)
        got_c.append(codes.clone())
        got_a.append(args.clone())
    got_c, got_a = torch.stack(got_c).cpu().numpy(), torch.stack(got_a).cpu().numpy()
    for k in range(K):
        want_c, want_a = fixture_commands(k, E)
        np.testing.assert_array_equal(got_c[k], want_c, err_msg=f"step {k}")
        np.testing.assert_allclose(got_a[k], want_a, rtol=0, atol=1e-12, err_msg=f"step {k}")


# ---- controller kernel, mixed ---------------------------------------------------------------------------------

def check_policy_rows(codes, args, n, pol, obs, t):
    """drone n's rows against DevicePolicy.act on a contiguous copy of its observation rows"""
    want = pol.act(obs[:, n].contiguous()).double()
    assert bool((codes[:, n] == COMMAND_CODE[Command.FULLSTATE]).all())
    assert torch.equal(args[:, n, 0:3], want[:, 0:3]) and torch.equal(args[:, n, 9], want[:, 3])
    assert bool((args[:, n, 13] == t).all())
    rest = [k for k in range(CMD_ARGS) if k not in (0, 1, 2, 9, 13)]
    assert bool((args[:, n][:, rest] == 0).all())
    # the numpy restatement of the row, on env 0
    code, row = R.policy_command_row(want[0].float().cpu().numpy(), t)
    assert int(codes[0, n]) == code and args[0, n].cpu().numpy().tolist() == row.tolist()


@pytest.mark.parametrize("E", [1, 70])
def test_mixed_controllers(E):
    """(hardcoded, policy A, None): the strided adrp_policy_act call (base obs + n D, rows E, stride N D) against
    the contiguous one, bit for bit; 70 rows are four 16-row tiles and a partial one"""
    N = 3
    obs0 = reset_obs("level0", E, N)
    D = obs0.shape[2]
    pol = random_policy(11)
    bank = ControllerBank(stub_env(E, N, D), ["hardcoded", pol, None])
    bank.reset(obs0)
    hc = HardCodedCommander(obs0)
    gen = torch.Generator(device="cuda").manual_seed(3)
    obs = obs0.clone()
    for k in list(range(4)) + [60, 61, 200, 420, 421, 422, 423]:
        t = k / 25
        codes, args = bank.predict(obs, t)
        want_c, want_a = hc.predict(t)
        assert torch.equal(codes[:, 0], want_c[:, 0]) and torch.equal(args[:, 0], want_a[:, 0]), f"step {k}"
        check_policy_rows(codes, args, 1, pol, obs, t)
        assert bool((codes[:, 2] == 0).all()) and bool((args[:, 2] == 0).all())
        # the next observation: anything a flight could show, so the relative setpoints move
        obs = obs0 + 0.5 * torch.randn(obs0.shape, generator=gen, device="cuda")
    assert torch.equal(bank.phase[:, :, 0].bool(), hc._flags[:, :, 0]) and not bool(bank.phase[:, :, 1:].any())
    pol.close()


def test_two_policies_with_different_weights():
    E, N = 37, 2
    obs0 = reset_obs("level0", E, N)
    a, b = random_policy(21, "relative"), random_policy(22, "absolute", hidden=32)
    bank = ControllerBank(stub_env(E, N, obs0.shape[2]), [a, b])
    bank.reset(obs0)
    gen = torch.Generator(device="cuda").manual_seed(4)
    for k in range(3):
        obs = obs0 + 0.5 * torch.randn(obs0.shape, generator=gen, device="cuda")
        codes, args = bank.predict(obs, k / 25)
        check_policy_rows(codes, args, 0, a, obs, k / 25)
        check_policy_rows(codes, args, 1, b, obs, k / 25)
    assert not torch.equal(args[:, 0, 0:3], args[:, 1, 0:3])
    a.close()
    b.close()


# ---- results kernel against the numpy restatement -------------------------------------------------------------

def feed(res, stream, base, n_open, ref=None):
    gate, flags, rew, term, trunc = stream
    dev = [torch.from_numpy(x).cuda() for x in stream]
    res.begin(base, n_open)
    if ref is not None:
        ref.begin(base, n_open)
    for t in range(gate.shape[0]):
        res.step_arrays(dev[0][t], dev[1][t], dev[2][t], dev[3][t], dev[4][t])
        if ref is not None:
            ref.step(gate[t], flags[t], rew[t], term[t], trunc[t])
            assert res.remaining() == ref.remaining, f"step {t}"


@pytest.mark.parametrize("E, N, n_open, base, C", [(1, 1, 1, 0, 1), (5, 2, 4, 3, 8), (130, 4, 130, 0, 130)])
def test_results_kernel_equals_the_restatement(E, N, n_open, base, C):
    """40 steps of constructed gate / flags / rew / term / trunc: env 0 closes on step 1, a drone is both
    eliminated and finished, env n_open - 1 never closes, (5, 2) is a last wave with n_open < E"""
    never = n_open - 1 if n_open > 1 else None
    stream = R.results_stream(40, E, N, seed=E, never=never)
    res, ref = RaceResults(E, N, C, 0), R.RaceAccounts(E, N, C)
    feed(res, stream, base, n_open, ref)
    both = (ref.run_finish >= 0) & (ref.run_elim >= 0)
    assert E == 1 or (both[1, 0] and ref.remaining >= 1 and ref.open[never])
    assert ref.log_length[base] == 1 and ref.logged >= 1
    assert res.meta.cpu().tolist() == [ref.logged, ref.remaining, ref.steps, 0]
    assert np.array_equal(res.log_return.cpu().numpy().view(np.int64), ref.log_return.view(np.int64))   # bit for bit
    assert np.array_equal(res.run_return.cpu().numpy().view(np.int64), ref.run_return.view(np.int64))
    for k in ("run_length", "run_gates", "run_finish", "run_elim", "log_length", "log_term", "log_trunc", "log_gates",
              "log_finish", "log_elim"):
        got, want = getattr(res, k).cpu().numpy(), getattr(ref, k)
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    assert np.array_equal(res.open.cpu().numpy().astype(bool), ref.open)
    assert np.array_equal(res.gates, ref.log_gates) and np.array_equal(res.finish_step, ref.log_finish)
    assert np.array_equal(res.winner, R.winner(ref.log_finish))
    assert np.array_equal(res.episode_times, ref.episode_times(25))
    # the same inputs again, into fresh buffers: the same bits
    again = RaceResults(E, N, C, 0)
    feed(again, stream, base, n_open)
    for k in DEVICE_BUFFERS:
        assert torch.equal(getattr(res, k), getattr(again, k)), k


def test_env_entry_reads_the_handle_image():
    """adrp_race_results_step_env against the handle-less entry fed from get_state()'s gate / flags rows, after
    every step of a scripted flight; gates and flags are planted in the state on the way so the rows differ"""
    E, N = 6, 2
    env = MultiRaceAviary("level0", num_drones=N, num_envs=E, seed=2, autoreset=False, commands=True)
    names = env.state_field_names()[1]
    gi, fi = names.index("gate"), names.index("flags")
    obs, _ = env.reset()
    hc = HardCodedCommander(obs)
    a, b = RaceResults(E, N, E, env.device, env.CTRL_FREQ), RaceResults(E, N, E, env.device, env.CTRL_FREQ)
    a.begin(0, E)
    b.begin(0, E)
    for k in range(30):
        if k == 10:
            f, i = env.get_state()
            i[gi] = torch.arange(E * N, dtype=torch.int32, device=env.device) % 4
            i[fi, 3] = 1                              # env 1, drone 1 eliminated
            env.set_state(f, i)
        obs, rew, term, trunc, _ = env.step(hc.predict(k / env.CTRL_FREQ))
        a.step(env, rew, term, trunc)
        _, i = env.get_state()
        b.step_arrays(i[gi].contiguous(), i[fi].contiguous(), rew, term, trunc)
        for name in DEVICE_BUFFERS:
            assert torch.equal(getattr(a, name), getattr(b, name)), f"step {k}: {name}"
    assert a.run_gates.cpu().flatten().tolist()[:4] != [0, 0, 0, 0] and int(a.run_elim[1, 1]) == 11
    assert a.run_length.cpu().tolist() == [30] * E
    env.close()


def test_env_entry_refuses_other_handles():
    """the two refusals that need a handle: a non-race one, and a race one of another shape"""
    from gym_pybullet_adrp_amd._lib import AdrpError
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    res = RaceResults(4, 2, 4, 0)
    res.begin(0, 4)
    before = [getattr(res, k).clone() for k in DEVICE_BUFFERS]
    hover = HoverAviary(num_envs=4)
    race = MultiRaceAviary("level0", num_drones=2, num_envs=3, autoreset=False)
    rew, flag = torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.bool, device="cuda")
    with pytest.raises(AdrpError, match="adrp_race_results_step_env: not a MultiRaceAviary handle"):
        res.step(hover, rew, flag, flag)
    with pytest.raises(AdrpError, match="adrp_race_results_step_env: the handle's E, N differ"):
        res.step(race, rew, flag, flag)
    assert all(torch.equal(getattr(res, k), b) for k, b in zip(DEVICE_BUFFERS, before))
    hover.close()
    race.close()


# ---- end to end -----------------------------------------------------------------------------------------------

def host_loop(n_runs, E, N=2):
    """simulate() built only from the pieces that were there before it: an autoreset=False env, the torch
    HardCodedCommander.predict, env.step((codes, args)) and get_state() flags fed to the numpy restatement"""
    env = MultiRaceAviary("level0", num_drones=N, num_envs=E, seed=0, autoreset=False, commands=True)
    names = env.state_field_names()[1]
    gi, fi = names.index("gate"), names.index("flags")
    acc = R.RaceAccounts(E, N, n_runs)
    for base in range(0, n_runs, E):
        obs, _ = env.reset()
        hc = HardCodedCommander(obs)
        acc.begin(base, min(E, n_runs - base))
        k = 0
        while acc.remaining > 0:
            assert k < 900
            obs, rew, term, trunc, _ = env.step(hc.predict(k / env.CTRL_FREQ))
            _, i = env.get_state()
            acc.step(i[gi].cpu().numpy(), i[fi].cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy())
            k += 1
    env.close()
    return acc


def results_tuple(res):
    return (res.episode_times.tolist(), res.episode_lengths.tolist(), res.episode_rewards.tolist(), res.gates.tolist(),
            res.finish_step.tolist(), res.elim_step.tolist(), res.winner.tolist(), res.terminated.tolist())


@pytest.fixture(scope="module")
def two_waves():
    return simulate("level0", ["hardcoded", "hardcoded"], n_runs=5, n_drones=2, num_envs=3, return_results=True)


def test_simulate_equals_the_host_loop(two_waves):
    """5 runs on 3 envs: two waves, the second with 2 open envs"""
    res, acc = two_waves, host_loop(5, 3)
    print("episode lengths", res.episode_lengths.tolist(), "finish", res.finish_step.tolist(), "winner", res.winner.tolist())
    assert res.logged() == 5 and res.remaining() == 0
    assert np.array_equal(res.episode_lengths, acc.log_length)
    assert np.array_equal(res.episode_times, acc.episode_times(25))
    assert np.array_equal(res.episode_rewards.view(np.int64), acc.log_return.view(np.int64))
    assert np.array_equal(res.gates, acc.log_gates) and np.array_equal(res.finish_step, acc.log_finish)
    assert np.array_equal(res.elim_step, acc.log_elim) and np.array_equal(res.winner, R.winner(acc.log_finish))
    assert np.array_equal(res.terminated, acc.log_term.astype(bool)) and np.array_equal(res.truncated, acc.log_trunc.astype(bool))
    ft = res.finish_times
    assert np.array_equal(np.isnan(ft), res.finish_step < 0)
    assert np.array_equal(ft[res.finish_step >= 0], (res.finish_step[res.finish_step >= 0] - 1) / 25)
    # the plain return value: the episode times in run order
    times = simulate("level0", ["hardcoded", "hardcoded"], n_runs=5, n_drones=2, num_envs=3)
    assert isinstance(times, list) and times == res.episode_times.tolist()


def test_simulate_does_not_depend_on_polling(two_waves):
    once = simulate("level0", ["hardcoded", "hardcoded"], n_runs=5, n_drones=2, num_envs=3, poll_every=1, return_results=True)
    assert results_tuple(once) == results_tuple(two_waves)


def test_simulate_one_wave_agrees_per_env(two_waves):
    """num_envs=5 covers the 5 runs in one wave.  An env's first episode depends on the seed and the env index
    alone, so runs 0..2 (envs 0..2 in both calls, each env's first episode) must be identical; runs 3 and 4 are
    the second episode of envs 0 and 1 in the 3-env call but the first of envs 3 and 4 here, and level0 draws every
    episode's start state, so they are only required to be complete."""
    one = simulate("level0", "hardcoded", n_runs=5, n_drones=2, num_envs=5, return_results=True)
    assert one.logged() == 5
    for got, want in zip(results_tuple(one), results_tuple(two_waves)):
        assert got[:3] == want[:3]
    assert (one.episode_lengths >= 1).all()


def test_simulate_max_steps(two_waves):
    longest = int(two_waves.episode_lengths.max())
    with pytest.raises(RuntimeError, match="still open"):
        simulate("level0", ["hardcoded", "hardcoded"], n_runs=5, n_drones=2, num_envs=3, max_steps=longest - 1)
    ok = simulate("level0", ["hardcoded", "hardcoded"], n_runs=5, n_drones=2, num_envs=3, max_steps=longest, return_results=True)
    assert results_tuple(ok) == results_tuple(two_waves)


def test_simulate_mixed_run():
    pol = random_policy(31)
    res = simulate("level0", ["hardcoded", pol], n_runs=4, n_drones=2, return_results=True)
    pol.close()
    n = res.episode_lengths
    print("mixed lengths", n.tolist(), "finish", res.finish_step.tolist(), "elim", res.elim_step.tolist())
    assert res.logged() == 4 and res.remaining() == 0 and (n >= 1).all()
    for v in (res.finish_step, res.elim_step):
        assert v.shape == (4, 2) and (((v == -1) | ((v >= 1) & (v <= n[:, None])))).all()
    assert ((res.terminated | res.truncated)).all()
