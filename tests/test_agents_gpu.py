"""The per-drone race agents kernels on the device (csrc/agents_kernel.h; include/adrp.h adrp_race_agents_*).
Needs an MI355X: -m gpu.

The yardstick is the numpy float64 restatement (tests/agents_reference.py, pinned by hand and against the oracle's
RewardWrapper in tests/test_agents_abi.py).  Everything but the reward is selects, copies and integer sums:
``valid``, ``next_start``, ``ep_length``, ``alive`` and ``wr_gate`` are compared exactly.  The reward is a float64
expression whose products and sums the device compiler may contract into fused multiply-adds and whose result is
rounded to float32 once: |kernel - ref| <= 2^-23 |ref| + 1e-12 for the rewards and the episode returns."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from tests import agents_reference as R  # noqa: E402

STATE = ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length")


class DeviceAgents:
    """the caller's side of adrp_race_agents_io, with one step's outputs"""

    def __init__(self, E, N, D, num_gates, device=0):
        self.lib = _lib.load()
        self.E, self.N, self.D = E, N, D
        self.device = torch.device("cuda", device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        R_ = E * N
        self.wr_gate, self.run_length = z(R_, torch.int32), z(R_, torch.int32)
        self.wr_target, self.wr_prev = z((R_, 3), torch.float64), z((R_, 3), torch.float64)
        self.alive, self.run_return = z(R_, torch.uint8), z(R_, torch.float64)
        self.rewards, self.next_start = z(R_, torch.float32), z(R_, torch.float32)
        self.valid, self.ep_return, self.ep_length = z(R_, torch.uint8), z(R_, torch.float64), z(R_, torch.int32)
        io = abi.AdrpRaceAgentsIO()
        io.struct_size = ctypes.sizeof(abi.AdrpRaceAgentsIO)
        io.num_envs, io.num_drones, io.obs_dim, io.num_gates = E, N, D, num_gates
        for k in STATE:
            setattr(io, k, getattr(self, k).data_ptr())
        self.io, self.ref = io, ctypes.byref(io)

    def _check(self, rc):
        if rc != 0:
            raise _lib.AdrpError(self.lib.adrp_last_error(None).decode())

    def _outs(self):
        return [t.data_ptr() for t in (self.rewards, self.valid, self.next_start, self.ep_return, self.ep_length)]

    def reset(self, obs, mask=None):
        self._check(self.lib.adrp_race_agents_reset(self.ref, obs.data_ptr(), None if mask is None else mask.data_ptr(),
                                                    _lib._raw_stream(self.device.index)))

    def step(self, obs, gate, flags, term, trunc, boot_value, gamma):
        self._check(self.lib.adrp_race_agents_step(self.ref, obs.data_ptr(), gate.data_ptr(), flags.data_ptr(), term.data_ptr(),
                                                   trunc.data_ptr(), boot_value.data_ptr(), gamma, *self._outs(),
                                                   _lib._raw_stream(self.device.index)))

    def step_env(self, env, obs, term, trunc, boot_value, gamma):
        self._check(self.lib.adrp_race_agents_step_env(self.ref, env.h.h, obs.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                                       boot_value.data_ptr(), gamma, *self._outs(),
                                                       _lib._raw_stream(self.device.index)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close_enough(got, want):
    """the bar of the module docstring: |k - ref| <= 2^-23 |ref| + 1e-12, NaN only where the reference has it"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bar = 2.0 ** -23 * np.abs(want[ok]) + 1e-12
    assert (err <= bar).all(), f"worst excess {float((err - bar).max()):.3e}"
    return float(err.max()) if err.size else 0.0


def check_state(k, ag, step):
    for name in ("alive", "wr_gate", "run_length"):
        assert np.array_equal(getattr(k, name).cpu().numpy(), getattr(ag, name)), f"step {step}: {name}"
    close_enough(k.run_return.cpu().numpy(), ag.run_return)
    # the target and the previous position are copies of float32 row values: exact
    assert np.array_equal(k.wr_target.cpu().numpy(), ag.wr_target), f"step {step}: wr_target"
    assert np.array_equal(k.wr_prev.cpu().numpy(), ag.wr_prev), f"step {step}: wr_prev"


@pytest.mark.parametrize("E, N, D, G", [(1, 1, 49, 4), (3, 2, 55, 4), (70, 3, 61, 4), (9, 8, 91, 2), (90, 3, 49, 4)])
def test_kernels_equal_the_restatement(E, N, D, G):
    """6 constructed steps through the array entry: gate passes, gate == num_gates, both flags on one drone, an
    elimination on the truncation step, envs that end and are reset by the mask, dead drones' rows (and stale
    bootstrap values, and the reset rows of envs that are not reset) all NaN / Inf.  (90, 3) is 270 lanes: a
    second block with a partial last wave; (9, 8) runs two gates, so a gate id at num_gates leaves the target."""
    first, steps = R.sequence(E, N, D, num_gates=G, T=6, seed=E + N)
    ag, k = R.Agents(E, N, D, G), DeviceAgents(E, N, D, G)
    # poison what a reset must rewrite, so a slot the kernel skipped shows
    k.alive.fill_(7)
    k.run_length.fill_(-5)
    ag.reset(first)
    k.reset(dev(first))
    check_state(k, ag, "reset")
    gamma, worst, dead = 0.97, 0.0, 0
    for t, s in enumerate(steps):
        was_alive = ag.alive != 0
        o = ag.step(s["obs"], s["gate"], s["flags"], s["term"], s["trunc"], s["boot_value"], gamma)
        k.step(dev(s["obs"]), dev(s["gate"]), dev(s["flags"]), dev(s["term"]), dev(s["trunc"]), dev(s["boot_value"]), gamma)
        rewards = k.rewards.cpu().numpy()
        assert np.array_equal(k.valid.cpu().numpy(), o["valid"]), f"step {t}: valid"
        assert np.array_equal(k.next_start.cpu().numpy(), o["next_start"]), f"step {t}: next_start"
        assert np.array_equal(k.ep_length.cpu().numpy(), o["ep_length"]), f"step {t}: ep_length"
        worst = max(worst, close_enough(rewards, o["stored"]), close_enough(k.ep_return.cpu().numpy(), o["ep_return"]))
        # a dead drone's poisoned row gives reward exactly 0 (bit pattern: +0)
        poisoned = ~was_alive & ~np.isfinite(s["obs"][:, 0])
        assert (rewards[poisoned].view(np.uint32) == 0).all()
        dead += int(poisoned.sum())
        check_state(k, ag, t)
        ag.reset(s["reset_obs"], s["mask"])
        k.reset(dev(s["reset_obs"]), dev(s["mask"]))
        check_state(k, ag, f"{t} reset")
    if E * N > 4:
        assert dead > 0
    print(f"E {E} N {N}: worst |kernel - restatement| {worst:.3e}")


def _set_rows(env, edits):
    """plant values in the race state: edits = [(field name, slot, value)]"""
    f, i = env.get_state()
    fn, inames = env.state_field_names()
    for name, slot, value in edits:
        if name in fn:
            f[fn.index(name), slot] = value
        else:
            i[inames.index(name), slot] = value
    env.set_state(f, i)


def test_one_drone_is_the_fused_wrapper():
    """N = 1: the agent's reward is the env's fused RewardWrapper reward (fp64 state) wherever the agent is valid,
    within 1e-5 absolute: the agents kernel reads the float32 rows, positions and targets under 3 m, so the two xy
    and the two z distance terms and the output roundings move it by <= ~3.6e-6.  Env 2 is given gate 1 in the
    state (the wrappers see a gate pass), env 5 is put outside the bounds (eliminated: the env terminates)."""
    E, T = 8, 40
    env = MultiRaceAviary("level0", num_drones=1, num_envs=E, seed=11, reward="wrapper", precision="fp64", autoreset=False)
    D = env.h.D
    k = DeviceAgents(E, 1, D, int(env.cfg.track.num_gates), env.device.index)
    obs, _ = env.reset()
    k.reset(obs)
    tv = torch.zeros(E, device=env.device)
    act = torch.cat([obs[..., :3] + torch.tensor([0.3, 0.2, 0.5], device=env.device), torch.zeros_like(obs[..., :1])], -1).contiguous()
    worst, passed, eliminated, resets = 0.0, 0, 0, 0
    for t in range(T):
        if t == 6:
            _set_rows(env, [("gate", 2, 1), ("pos_x", 5, float(env.cfg.track.bounds_hi[0]) + 1.0)])
        obs, rew, term, trunc, _ = env.step(act)
        k.step_env(env, obs, term, trunc, tv, 0.99)
        valid = k.valid.bool()
        assert bool(valid.all())                     # every env is reset on the step it ends: no dead slot with N = 1
        err = float((k.rewards - rew).abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, f"step {t}: {err:.3e}"
        _, i = env.get_state()
        names = env.state_field_names()[1]
        flags = i[names.index("flags")]
        passed += int((rew > 4).sum())
        eliminated += int(((flags & 1) != 0).sum())
        assert torch.equal(k.next_start.bool(), term | trunc) and torch.equal((flags & 3) != 0, term)
        mask = (term | trunc).to(torch.uint8)
        resets += int(mask.sum())
        obs, _ = env.reset(mask=mask)
        k.reset(obs, mask)
    assert passed >= 1 and eliminated >= 1 and resets >= 1
    print(f"N = 1: worst |agent reward - fused wrapper reward| {worst:.3e}")
    env.close()


def test_env_entry_reads_the_handle_image_and_refuses_other_handles():
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    E, N = 6, 2
    env = MultiRaceAviary("level0", num_drones=N, num_envs=E, seed=2, autoreset=False)
    D = env.h.D
    a, b = DeviceAgents(E, N, D, 4), DeviceAgents(E, N, D, 4)
    obs, _ = env.reset()
    a.reset(obs)
    b.reset(obs)
    act = torch.cat([obs[..., :3] + 0.2, torch.zeros_like(obs[..., :1])], -1).contiguous()
    tv = torch.full((E * N,), 2.0, device=env.device)
    names = env.state_field_names()[1]
    for t in range(4):
        if t == 1:
            _set_rows(env, [("gate", 3, 2), ("flags", 7, 1), ("flags", 8, 2), ("gate", 8, 4)])
        obs, _, term, trunc, _ = env.step(act)
        a.step_env(env, obs, term, trunc, tv, 0.9)
        _, i = env.get_state()
        b.step(obs, i[names.index("gate")].contiguous(), i[names.index("flags")].contiguous(), term, trunc, tv, 0.9)
        for name in STATE + ("rewards", "valid", "next_start", "ep_length"):
            assert torch.equal(getattr(a, name), getattr(b, name)), f"step {t}: {name}"
        assert torch.equal(a.ep_return.view(torch.int64), b.ep_return.view(torch.int64))
    assert a.alive.cpu().tolist()[7:9] == [0, 0] and int(a.wr_gate[3]) == 2
    before = [getattr(a, name).clone() for name in STATE]
    hover = HoverAviary(num_envs=E)
    other = MultiRaceAviary("level0", num_drones=N, num_envs=E + 1, autoreset=False)
    with pytest.raises(_lib.AdrpError, match="adrp_race_agents_step_env: not a MultiRaceAviary handle"):
        a.step_env(hover, obs, term, trunc, tv, 0.9)
    with pytest.raises(_lib.AdrpError, match="adrp_race_agents_step_env: the handle's E, N, D differ"):
        a.step_env(other, obs, term, trunc, tv, 0.9)
    assert all(torch.equal(getattr(a, name), x) for name, x in zip(STATE, before))
    for e in (env, hover, other):
        e.close()
