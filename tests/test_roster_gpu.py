"""The race roster kernels on the device (csrc/roster_kernel.h; include/adrp.h adrp_race_roster_*), called directly
on constructed inputs.  Needs an MI355X: -m gpu.

Yardsticks: the numpy float64 restatement (tests/roster_reference.py, pinned by hand in tests/test_roster_abi.py),
and the two launches that were there before, which run the same device functions (csrc/race_slot.h):
``adrp_race_controllers`` with a scalar episode time for the act launch, ``adrp_race_agents_step`` for the compact
step.  The act launch is copies, selects and one IEEE float64 division: codes, args and phase are compared with
``torch.equal``.  So are the compact step's outputs against the full-width launch; against the restatement the
bars are tests/test_agents_gpu.py's (ints exact, rewards and episode returns within 2^-23 |ref| + 1e-12)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from tests import agents_reference as A  # noqa: E402
from tests import roster_reference as R  # noqa: E402
from tests.test_agents_gpu import STATE, DeviceAgents, close_enough, dev  # noqa: E402

L_, H_, P_, N_ = R.LEARNER, R.HARDCODED, R.POLICY, R.NONE
# (90, 3) is 270 slots: a second block with a partial last wave
SHAPES = [(1, 1, [L_]), (3, 2, [H_, L_]), (9, 8, [L_, H_, P_, N_, L_, H_, P_, L_]), (90, 3, [P_, H_, L_])]
REF_LEN = 6


class DeviceRoster:
    """the caller's side of adrp_race_roster_io"""

    def __init__(self, E, N, roles, ctrl_freq, seed=0):
        self.lib = _lib.load()
        self.E, self.N, self.roles, self.ctrl_freq = E, N, list(roles), float(ctrl_freq)
        self.learners = R.learners_of(roles)
        self.L = len(self.learners)
        rng = np.random.default_rng(seed)
        self.ref = dev(rng.uniform(-3, 3, (E, N, REF_LEN, 3)))
        self.offset = dev(rng.integers(0, 5, (E, N)).astype(np.int64))
        self.setpoints = dev(rng.uniform(-3, 3, (N, E, 4)).astype(np.float32))
        self.learner_act = dev(rng.uniform(-3, 3, (self.L, E, 4)).astype(np.float32))
        self.clock = torch.zeros(E, dtype=torch.int32, device="cuda")
        self.phase = torch.zeros((3, E * N), dtype=torch.uint8, device="cuda")
        # poisoned: every slot is written on every call
        self.codes = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
        self.args = torch.full((E, N, abi.CMD_ARGS), float("nan"), dtype=torch.float64, device="cuda")
        io = abi.AdrpRaceRosterIO()
        io.struct_size = ctypes.sizeof(abi.AdrpRaceRosterIO)
        io.num_envs, io.num_drones, io.num_learners, io.ref_len, io.ctrl_freq = E, N, self.L, REF_LEN, self.ctrl_freq
        for n, r in enumerate(roles):
            io.role[n] = r
            io.learner_index[n] = self.learners.index(n) if r == L_ else -1
        for k in ("clock", "phase", "ref", "offset", "setpoints", "learner_act", "codes", "args"):
            setattr(io, k, getattr(self, k).data_ptr())
        self.io, self.ptr = io, ctypes.byref(io)

    def _check(self, rc):
        if rc != 0:
            raise _lib.AdrpError(self.lib.adrp_last_error(None).decode())

    def act(self):
        self._check(self.lib.adrp_race_roster_act(self.ptr, _lib._raw_stream(0)))

    def tick(self, mask=None):
        self._check(self.lib.adrp_race_roster_tick(self.ptr, None if mask is None else mask.data_ptr(), _lib._raw_stream(0)))

    def restatement(self):
        ro = R.Roster(self.E, self.N, self.roles, self.ctrl_freq, self.ref.cpu().numpy(), self.offset.cpu().numpy())
        ro.clock[:] = self.clock.cpu().numpy()
        ro.phase[:] = self.phase.cpu().numpy()
        return ro

    def step(self, ag, out, obs, gate, flags, term, trunc, boot_value, gamma):
        """ag: DeviceAgents (the E N state); out: DeviceAgents-like holder of [L E] outputs"""
        self._check(self.lib.adrp_race_roster_step(self.ptr, ag.ref, obs.data_ptr(), gate.data_ptr(), flags.data_ptr(),
                                                   term.data_ptr(), trunc.data_ptr(), boot_value.data_ptr(), gamma, *out.ptrs(),
                                                   _lib._raw_stream(0)))


def controllers_twin(k, clock_value, phase0):
    """adrp_race_controllers on the same tables with the scalar clock_value / ctrl_freq, LEARNER drones presented as
    POLICY drones fed from the same setpoints -> codes, args, phase"""
    E, N = k.E, k.N
    sp = k.setpoints.clone()
    for l, n in enumerate(k.learners):
        sp[n] = k.learner_act[l]
    codes = torch.full((E, N), -7, dtype=torch.int32, device="cuda")
    args = torch.full((E, N, abi.CMD_ARGS), float("nan"), dtype=torch.float64, device="cuda")
    phase = phase0.clone()
    io = abi.AdrpRaceCtrlIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceCtrlIO)
    io.num_envs, io.num_drones, io.ref_len = E, N, REF_LEN
    for n, r in enumerate(k.roles):
        io.kind[n] = abi.RACE_CTRL_POLICY if r == L_ else r
    io.ref, io.offset, io.phase, io.setpoints = k.ref.data_ptr(), k.offset.data_ptr(), phase.data_ptr(), sp.data_ptr()
    io.codes, io.args = codes.data_ptr(), args.data_ptr()
    rc = k.lib.adrp_race_controllers(ctypes.byref(io), clock_value / k.ctrl_freq, _lib._raw_stream(0))
    assert rc == 0, k.lib.adrp_last_error(None).decode()
    torch.cuda.synchronize()
    return codes, args, phase


def bits64(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("ctrl_freq", [25, 30])
@pytest.mark.parametrize("E, N, roles", SHAPES)
def test_act_equals_the_restatement_and_the_scalar_clock_launch(E, N, roles, ctrl_freq):
    """per-env clocks from 0 over the step == L edge (offsets 0..4, L = 6: steps -4..) to far past landing, every
    combination of the three phase flags; two calls, so the flags the first one set are read by the second"""
    k = DeviceRoster(E, N, roles, ctrl_freq, seed=E + N)
    clocks = np.array([0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 40, 3, 1000])
    k.clock.copy_(dev(clocks[(np.arange(E) * 7) % len(clocks)].astype(np.int32)))
    combos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 0, 1], [0, 1, 1], [0, 1, 0], [0, 0, 1]], np.uint8)
    k.phase.copy_(dev(np.ascontiguousarray(combos[(np.arange(E * N) * 3 + E) % 8].T)))
    seen = set()
    for call in range(2):
        ro, phase0 = k.restatement(), k.phase.clone()
        k.codes.fill_(-7)
        k.args.fill_(float("nan"))
        k.act()
        want_codes, want_args = ro.act(k.setpoints.cpu().numpy(), k.learner_act.cpu().numpy())
        assert torch.equal(k.codes, dev(want_codes)), f"call {call}: codes"
        assert torch.equal(bits64(k.args), bits64(dev(want_args))), f"call {call}: args"
        assert torch.equal(k.phase, dev(ro.phase)), f"call {call}: phase"
        assert torch.equal(k.clock, dev(ro.clock))                                   # only read
        seen |= set(want_codes.reshape(-1).tolist())
        # the launch that was there before, one scalar clock at a time
        clock = k.clock.cpu().numpy()
        for value in np.unique(clock):
            codes, args, phase = controllers_twin(k, int(value), phase0)
            rows = dev(np.nonzero(clock == value)[0])
            assert torch.equal(k.codes[rows], codes[rows]), f"call {call}, clock {value}: codes"
            assert torch.equal(bits64(k.args[rows]), bits64(args[rows])), f"call {call}, clock {value}: args"
            assert torch.equal(k.phase.view(3, E, N)[:, rows], phase.view(3, E, N)[:, rows]), f"call {call}, clock {value}: phase"
        k.tick(dev((np.arange(E) % 4 == 3).astype(np.uint8)))
    if E == 90:          # its roster has no NONE drone: code 0 is a scripted drone past its landing
        assert {R.CMD_TAKEOFF, R.CMD_FULLSTATE, R.CMD_NOTIFY, R.CMD_LAND, R.CMD_NONE} <= seen, seen


@pytest.mark.parametrize("E, N, roles", SHAPES)
def test_tick(E, N, roles):
    """masks: NULL (every env), none, all and a ragged pattern; clocks and flags exact"""
    k = DeviceRoster(E, N, roles, 25)
    rng = np.random.default_rng(E)
    k.clock.copy_(dev(rng.integers(0, 50, E).astype(np.int32)))
    k.phase.copy_(dev(rng.integers(0, 2, (3, E * N)).astype(np.uint8)))
    ragged = ((np.arange(E) * 5) % 3 == 0).astype(np.uint8)
    for mask in (np.zeros(E, np.uint8), ragged, 2 * ragged[::-1].copy(), np.ones(E, np.uint8), None):
        ro = k.restatement()
        ro.tick(mask)
        k.tick(None if mask is None else dev(mask))
        assert torch.equal(k.clock, dev(ro.clock)) and torch.equal(k.phase, dev(ro.phase))
        if mask is None or mask.all():
            assert not k.clock.any() and not k.phase.any()
        # something to clear and to count for the next mask
        k.clock.add_(dev(np.arange(E, dtype=np.int32) % 3))
        k.phase.copy_(dev(rng.integers(0, 2, (3, E * N)).astype(np.uint8)))
    before = k.clock.clone()
    k.tick(dev(np.zeros(E, np.uint8)))
    assert torch.equal(k.clock, before + 1)


class Outputs:
    """one step's [L E] outputs"""

    def __init__(self, cols):
        z = lambda dt: torch.zeros(cols, dtype=dt, device="cuda")
        self.rewards, self.next_start = z(torch.float32), z(torch.float32)
        self.valid, self.ep_return, self.ep_length = z(torch.uint8), z(torch.float64), z(torch.int32)

    def ptrs(self):
        return [t.data_ptr() for t in (self.rewards, self.valid, self.next_start, self.ep_return, self.ep_length)]


@pytest.mark.parametrize("E, N, roles", SHAPES)
def test_compact_step_equals_the_full_width_launch_and_the_restatement(E, N, roles):
    """6 constructed steps (tests/agents_reference.py sequence: gate passes, eliminations, finishes, truncations with
    a bootstrap, envs reset by the mask; a dead drone's rows and every stale boot_value NaN / Inf).  The compact
    launch works on state ``k``, the full-width one on its twin ``f``; column l E + e against slot e N + drone_l."""
    D, G, gamma = 49 + 2 * N, 4, 0.97
    first, steps = A.sequence(E, N, D, num_gates=G, T=6, seed=3 * E + N)
    ro = DeviceRoster(E, N, roles, 25)
    L = ro.L
    slot = np.array([[e * N + n for e in range(E)] for n in ro.learners]).reshape(L * E)      # column -> slot
    slot_d = dev(slot)
    others = dev(np.setdiff1d(np.arange(E * N), slot))
    ag, k, f = A.Agents(E, N, D, G), DeviceAgents(E, N, D, G), DeviceAgents(E, N, D, G)
    out = Outputs(L * E)
    ag.reset(first)
    k.reset(dev(first))
    f.reset(dev(first))
    seen = dict(passed=0, eliminated=0, finished=0, boot=0, dead=0, reset=0)
    worst = 0.0
    for t, s in enumerate(steps):
        was_alive, gate_before = ag.alive[slot] != 0, ag.wr_gate[slot].copy()
        # boot_value [L E]: the full-width one's learner slots (NaN wherever the env is not truncated)
        boot = s["boot_value"][slot]
        o = R.compact_step(ag, ro.learners, s["obs"], s["gate"], s["flags"], s["term"], s["trunc"], boot, gamma)
        inputs = [dev(s[x]) for x in ("obs", "gate", "flags", "term", "trunc")]
        before = [getattr(k, name)[others].clone() for name in STATE]
        for x in (out.rewards, out.next_start, out.ep_return):
            x.fill_(float("nan"))
        ro.step(k, out, *inputs, dev(boot), gamma)
        f.step(*inputs, dev(s["boot_value"]), gamma)
        # the full-width launch at the learner slots: equality, state included
        for name in ("rewards", "valid", "next_start", "ep_length"):
            assert torch.equal(getattr(out, name), getattr(f, name)[slot_d]), f"step {t}: {name}"
        assert torch.equal(bits64(out.ep_return), bits64(f.ep_return[slot_d])), f"step {t}: ep_return"
        assert torch.equal(out.rewards.view(torch.int32), f.rewards[slot_d].view(torch.int32))
        for name in STATE:
            assert torch.equal(getattr(k, name)[slot_d], getattr(f, name)[slot_d]), f"step {t}: {name}"
        # the other slots' state is not touched
        for name, x in zip(STATE, before):
            assert torch.equal(getattr(k, name)[others], x), f"step {t}: {name} of a slot that is no learner's"
        # the restatement
        for name in ("valid", "next_start", "ep_length"):
            assert np.array_equal(getattr(out, name).cpu().numpy(), o[name]), f"step {t}: {name}"
        rewards = out.rewards.cpu().numpy()
        worst = max(worst, close_enough(rewards, o["stored"]), close_enough(out.ep_return.cpu().numpy(), o["ep_return"]))
        for name in ("alive", "wr_gate", "run_length"):
            assert np.array_equal(getattr(k, name).cpu().numpy()[slot], getattr(ag, name)[slot]), f"step {t}: {name}"
        poisoned = ~was_alive & ~np.isfinite(s["obs"][slot, 0])
        assert (rewards[poisoned].view(np.uint32) == 0).all()
        fl = s["flags"][slot]
        seen["passed"] += int((was_alive & (ag.wr_gate[slot] > gate_before)).sum())
        seen["eliminated"] += int((was_alive & ((fl & 1) != 0)).sum())
        seen["finished"] += int((was_alive & ((fl & 2) != 0)).sum())
        seen["boot"] += int(o["boot"].sum())
        seen["dead"] += int(poisoned.sum())
        seen["reset"] += int(s["mask"].sum())
        ag.reset(s["reset_obs"], s["mask"])
        k.reset(dev(s["reset_obs"]), dev(s["mask"]))
        f.reset(dev(s["reset_obs"]), dev(s["mask"]))
    if L * E > 4:
        assert all(v > 0 for v in seen.values()), seen
    print(f"E {E} N {N} L {L}: worst |kernel - restatement| {worst:.3e}; {seen}")


def test_env_entry_reads_the_handle_image_and_refuses_other_handles():
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    E, N, roles = 6, 3, [H_, L_, L_]
    env = MultiRaceAviary("level0", num_drones=N, num_envs=E, seed=2, autoreset=False)
    D = env.h.D
    ro = DeviceRoster(E, N, roles, env.CTRL_FREQ)
    a, b = DeviceAgents(E, N, D, 4), DeviceAgents(E, N, D, 4)
    oa, ob = Outputs(2 * E), Outputs(2 * E)
    obs, _ = env.reset()
    a.reset(obs)
    b.reset(obs)
    act = torch.cat([obs[..., :3] + 0.2, torch.zeros_like(obs[..., :1])], -1).contiguous()
    tv = torch.full((2 * E,), 2.0, device=env.device)
    names = env.state_field_names()[1]

    def step_env(handle_env):
        ro._check(ro.lib.adrp_race_roster_step_env(ro.ptr, a.ref, handle_env.h.h, obs.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                                   tv.data_ptr(), 0.9, *oa.ptrs(), _lib._raw_stream(0)))

    for t in range(4):
        if t == 1:
            f, i = env.get_state()
            i[names.index("gate"), 4] = 2
            i[names.index("flags"), 7] = 1
            i[names.index("flags"), 8] = 2
            i[names.index("gate"), 8] = 4
            env.set_state(f, i)
        obs, _, term, trunc, _ = env.step(act)
        step_env(env)
        _, i = env.get_state()
        ro.step(b, ob, obs, i[names.index("gate")].contiguous(), i[names.index("flags")].contiguous(), term, trunc, tv, 0.9)
        for name in STATE:
            assert torch.equal(getattr(a, name), getattr(b, name)), f"step {t}: {name}"
        for name in ("rewards", "valid", "next_start", "ep_length"):
            assert torch.equal(getattr(oa, name), getattr(ob, name)), f"step {t}: {name}"
        assert torch.equal(bits64(oa.ep_return), bits64(ob.ep_return))
    assert a.alive.cpu().tolist()[7:9] == [0, 0] and int(a.wr_gate[4]) == 2 and int(a.run_length[0]) == 0
    before = [getattr(a, name).clone() for name in STATE]
    hover = HoverAviary(num_envs=E)
    other = MultiRaceAviary("level0", num_drones=N, num_envs=E + 1, autoreset=False)
    with pytest.raises(_lib.AdrpError, match="adrp_race_roster_step_env: not a MultiRaceAviary handle"):
        step_env(hover)
    with pytest.raises(_lib.AdrpError, match="adrp_race_roster_step_env: the handle's E, N, D differ"):
        step_env(other)
    assert all(torch.equal(getattr(a, name), x) for name, x in zip(STATE, before))
    for e in (env, hover, other):
        e.close()
