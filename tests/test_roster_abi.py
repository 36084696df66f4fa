"""C-ABI surface of the race rosters (include/adrp.h adrp_race_roster_*, csrc/roster.hip), the part that needs no
GPU: the header / library / ctypes mirror agree, every refusal is reached without a device and names the function
and its cause, and the numpy yardstick (tests/roster_reference.py) on a case computed by hand.

Two refusals of adrp_race_roster_step_env need a handle to refuse (a non-race one, a race one of another shape);
creating a handle needs a device, so they are in tests/test_roster_gpu.py.  The NULL handle is refused here."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_pybullet_adrp_amd import _lib
from gym_pybullet_adrp_amd.utils import abi
from tests import agents_reference as A
from tests import roster_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROSTER_FUNCTIONS = {"adrp_race_roster_act", "adrp_race_roster_tick", "adrp_race_roster_step", "adrp_race_roster_step_env"}
BUFFERS = ("clock", "phase", "ref", "offset", "setpoints", "learner_act", "codes", "args")
AGENT_BUFFERS = ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length")
PTR = 0x1000        # never dereferenced: every call below is refused before the first device call


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_roster_functions(lib):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src) if f.startswith("adrp_race_roster_")}
    assert declared == ROSTER_FUNCTIONS
    assert not [f for f in declared if not hasattr(lib, f)]
    assert "#define ADRP_ABI_VERSION 2" in text           # purely additive: the ABI version stays
    assert lib.adrp_abi_version() == 2
    for name in ("NONE", "HARDCODED", "POLICY", "LEARNER"):
        assert f"#define ADRP_ROSTER_{name} {getattr(abi, 'ROSTER_' + name)}" in text
        assert getattr(R, name) == getattr(abi, "ROSTER_" + name)
    # the first three roles are the race evaluation's kinds
    assert (abi.ROSTER_NONE, abi.ROSTER_HARDCODED, abi.ROSTER_POLICY) == (abi.RACE_CTRL_NONE, abi.RACE_CTRL_HARDCODED,
                                                                         abi.RACE_CTRL_POLICY)


def test_struct_mirror():
    """the header's struct on LP64: six 32-bit fields, a double, two int32 [8] arrays, eight pointers; the structs
    that were there keep their sizes"""
    assert ctypes.sizeof(abi.AdrpRaceRosterIO) == 6 * 4 + 8 + 2 * 8 * 4 + 8 * 8
    assert abi.AdrpRaceRosterIO.ctrl_freq.offset == 24 and abi.AdrpRaceRosterIO.clock.offset == 96
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    body = re.search(r"typedef struct adrp_race_roster_io \{(.*?)\} adrp_race_roster_io;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f[0] for f in abi.AdrpRaceRosterIO._fields_]
    assert re.findall(r"(\w+)(?:\[\w+\])?\s*;", body) == fields
    assert fields[9:] == list(BUFFERS)
    assert ctypes.sizeof(abi.AdrpRaceAgentsIO) == 6 * 4 + 6 * 8 and ctypes.sizeof(abi.AdrpRaceCtrlIO) == 4 * 4 + 8 * 4 + 6 * 8


def _io(roles=(3, 1, 2), index=None, **change):
    io = abi.AdrpRaceRosterIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceRosterIO)
    io.num_envs, io.num_drones, io.ref_len, io.ctrl_freq = 5, len(roles), 300, 25.0
    io.num_learners = sum(r == abi.ROSTER_LEARNER for r in roles)
    learners = [n for n, r in enumerate(roles) if r == abi.ROSTER_LEARNER]
    for n, r in enumerate(roles):
        io.role[n] = r
        io.learner_index[n] = learners.index(n) if r == abi.ROSTER_LEARNER else -1
    for n, l in (index or {}).items():
        io.learner_index[n] = l
    for k in BUFFERS:
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


def _agents(**change):
    io = abi.AdrpRaceAgentsIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceAgentsIO)
    io.num_envs, io.num_drones, io.obs_dim, io.num_gates = 5, 3, 55, 4
    for k in AGENT_BUFFERS:
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


def _calls(lib, io, agents=None, which=ROSTER_FUNCTIONS):
    ref = None if io is None else ctypes.byref(io)
    ag = ctypes.byref(agents if agents is not None else _agents(num_drones=io.num_drones if io is not None else 3))
    calls = (("adrp_race_roster_act", lambda: lib.adrp_race_roster_act(ref, None)),
             ("adrp_race_roster_tick", lambda: lib.adrp_race_roster_tick(ref, PTR, None)),
             ("adrp_race_roster_step", lambda: lib.adrp_race_roster_step(ref, ag, *[PTR] * 6, 0.99, *[PTR] * 5, None)),
             ("adrp_race_roster_step_env", lambda: lib.adrp_race_roster_step_env(ref, ag, PTR, *[PTR] * 4, 0.99, *[PTR] * 5, None)))
    return [c for c in calls if c[0] in which]


def _refused(lib, calls, word):
    for fn, call in calls:
        assert call() == abi.ERR_INVALID, fn
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith(fn + ":") and word in msg, msg


L_, H_, P_, N_ = abi.ROSTER_LEARNER, abi.ROSTER_HARDCODED, abi.ROSTER_POLICY, abi.ROSTER_NONE
# refused by all four entry points: the roster itself
ROSTER_REFUSALS = [
    (_io(struct_size=8), "struct_size"), (_io(struct_size=ctypes.sizeof(abi.AdrpRaceRosterIO) + 8), "struct_size"),
    (_io(num_envs=0), "num_envs"), (_io(num_envs=-3), "num_envs"),
    (_io(num_drones=0), "num_drones"), (_io(num_drones=abi.MAX_DRONES + 1), "num_drones"),
    (_io(num_learners=0), "num_learners"), (_io(num_learners=4), "num_learners"), (_io((N_, H_)), "num_learners"),
    (_io((L_, 4)), "role must be"), (_io((L_, -1)), "role must be"),
    (_io((L_, H_), index={1: 0}), "learner_index must be -1"),               # >= 0 on another role
    (_io((L_, L_), index={1: 0}), "the same index"),                          # not injective
    (_io((L_, L_), index={1: 2}), "0..num_learners-1"),                       # past L - 1
    (_io((L_, L_), index={0: -1}), "0..num_learners-1"),                      # a learner without an index
    (_io((L_, L_, N_), num_learners=1), "0..num_learners-1"),                 # more LEARNER drones than L
    (_io((L_, N_, N_), num_learners=2), "not num_learners"),                  # fewer
]
# refused by act and tick: what their launches read
BUFFER_REFUSALS = [
    (_io(ctrl_freq=0.0), "ctrl_freq"), (_io(ctrl_freq=-25.0), "ctrl_freq"), (_io(ctrl_freq=float("nan")), "ctrl_freq"),
    (_io(clock=None), "NULL buffer"), (_io(phase=None), "NULL buffer"), (_io(codes=None), "NULL buffer"),
    (_io(args=None), "NULL buffer"), (_io(args=PTR + 8), "16-byte aligned"),
    (_io(ref=None), "HARDCODED"), (_io(offset=None), "HARDCODED"), (_io(ref_len=0), "HARDCODED"),
    (_io(setpoints=None), "POLICY"), (_io(learner_act=None), "LEARNER"),
]


@pytest.mark.parametrize("io, word", ROSTER_REFUSALS)
def test_roster_refusals(lib, io, word):
    """checked before any device call (and before the agents io or the handle is looked at): they answer without a GPU"""
    _refused(lib, _calls(lib, io), word)


@pytest.mark.parametrize("io, word", BUFFER_REFUSALS)
def test_buffer_refusals(lib, io, word):
    _refused(lib, _calls(lib, io, which=("adrp_race_roster_act", "adrp_race_roster_tick")), word)


def test_null_and_step_refusals(lib):
    for fn, call in _calls(lib, None):
        assert call() == abi.ERR_INVALID
        assert lib.adrp_last_error(None).decode() == f"{fn}: io is NULL"
    io = _io()
    ref = ctypes.byref(io)
    step = ("adrp_race_roster_step", "adrp_race_roster_step_env")
    for fn in step:
        args = [PTR] * (10 if fn.endswith("_env") else 11)
        assert getattr(lib, fn)(ref, None, *args[:-5], 0.99, *args[-5:], None) == abi.ERR_INVALID
        assert lib.adrp_last_error(None).decode() == f"{fn}: the agents io is NULL"
    for change, word in ((dict(struct_size=8), "adrp_race_agents_io.struct_size"), (dict(num_envs=6), "differ from the roster's"),
                         (dict(num_drones=2), "differ from the roster's"), (dict(obs_dim=48), "obs_dim"),
                         (dict(num_gates=5), "num_gates"), (dict(alive=None), "NULL buffer"), (dict(wr_prev=None), "NULL buffer")):
        _refused(lib, _calls(lib, io, _agents(**change), which=step), word)
    ag = ctypes.byref(_agents())
    for k in range(11):
        args = [PTR] * 11
        args[k] = None
        assert lib.adrp_race_roster_step(ref, ag, *args[:6], 0.99, *args[6:], None) == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith("adrp_race_roster_step:") and "NULL" in msg
        assert ("obs / gate / flags / term / trunc / boot_value" if k < 6 else
                "rewards / valid / next_start / ep_return / ep_length") in msg
    assert lib.adrp_race_roster_step_env(ref, ag, None, *[PTR] * 4, 0.99, *[PTR] * 5, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_roster_step_env: the handle is NULL"


def _row(pos, gate, D=49):
    """an obs row: the position, the four gates at (3,4,1) (6,8,1) (0,0,1) (0,0,1), the gate id in column 48"""
    row = np.zeros(D, np.float32)
    row[0:3] = pos
    row[12:28] = [3, 4, 1, 0, 6, 8, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    row[48] = gate
    return row


def test_reference_by_hand():
    """2 envs x 3 drones, roles learner / hardcoded / none, ctrl_freq 25, gamma 0.5.  The scripted drone's table has
    L = 2 samples, (1, 2, 3) and (4, 5, 6) in env 0, ten times that in env 1, and offset 1.  Four steps; env 1 is
    truncated at the second and reset, so from the third the clocks differ.

    commands (drone 0: FULLSTATE of its learner_act; drone 1 scripted; drone 2 NONE, zeros), ep_time = clock / 25:
    step 0  clocks 0, 0: both scripted drones TAKEOFF [0.3, 2], time slot 2.
    step 1  clocks 1, 1: trunc(0.04 * 25) - 1 = 0: FULLSTATE ref[0], acc 0.5, time 0.04.
    step 2  clocks 2, 0: env 0 FULLSTATE ref[1] at 0.08; env 1 takes off again.
    step 3  clocks 3, 1: env 0 step 2 = L: NOTIFY [0.12]; env 1 FULLSTATE ref[0] at 0.04.
    a fifth act at clocks 4, 2: env 0 LAND [0, 2]; env 1 FULLSTATE ref[1] at 0.08.  A sixth: env 0 NONE; env 1 NOTIFY.

    learner columns (column e; every drone reset at (0, 0, 1), gate 0, target (3, 4, 1)):
    step 0  env 0 flies to (1.5, 2, 1): 5 -> 2.5, reward 2.5.  env 1 stays: 0.
    step 1  env 0 reaches (3, 4, 1) and passes gate 0: the target becomes (6, 8, 1), 7.5 -> 5, + 5: 7.5.
            env 1 is truncated: raw 0, stored 0 + 0.5 * 3 = 1.5, episode (0, 2); reset by the mask.
    step 2  env 0 drops to (3, 4, 0.5), eliminated: 0 - 0.5 - 1 = -1.5, episode (8.5, 3).  env 1 to (1.5, 2, 1): 2.5.
    step 3  env 0's learner is dead: NaN row, reward 0, not valid, start 1.  env 1 to (3, 4, 1) without a gate: 2.5.
    The scripted and the idle drone's agent slots keep their reset state throughout, whatever their rows hold."""
    nan = np.nan
    E, N, roles = 2, 3, [R.LEARNER, R.HARDCODED, R.NONE]
    ref = np.zeros((E, N, 2, 3))
    ref[0, 1], ref[1, 1] = [[1, 2, 3], [4, 5, 6]], [[10, 20, 30], [40, 50, 60]]
    ro = R.Roster(E, N, roles, 25.0, ref, np.ones((E, N), np.int64))
    assert ro.learners == [0] and R.learners_of([3, 0, 3, 1]) == [0, 2]
    ag = A.Agents(E, N, 49, 4)
    start = np.stack([_row((0, 0, 1), 0)] * 6)
    ag.reset(start)
    ro.tick(None)
    act = np.arange(8, dtype=np.float32).reshape(1, 2, 4) + 0.5         # learner_act [L = 1][E][4]
    junk = np.full(49, nan, np.float32)

    def cmd(code, **slots):
        a = np.zeros(14)
        for k, v in slots.items():
            a[int(k[1:])] = v
        return code, a.tolist()

    def check(want):
        codes, args = ro.act(None, act)
        for e in range(E):
            assert (codes[e, 0], args[e, 0].tolist()) == cmd(1, a0=act[0, e, 0], a1=act[0, e, 1], a2=act[0, e, 2],
                                                              a9=act[0, e, 3], a13=ro.clock[e] / 25.0)
            assert (codes[e, 1], args[e, 1].tolist()) == want[e], (e, codes[e, 1], args[e, 1])
            assert (codes[e, 2], args[e, 2].tolist()) == cmd(0)

    def step(rows, gate, flags, term, trunc, boot):
        return R.compact_step(ag, ro.learners, np.stack(rows), gate, flags, term, trunc, boot, 0.5)

    takeoff = cmd(2, a0=0.3, a1=2.0, a13=2.0)
    # step 0
    check([takeoff, takeoff])
    assert ro.phase.tolist() == [[0, 1, 0, 0, 1, 0], [0] * 6, [0] * 6]
    o = step([_row((1.5, 2, 1), 0), junk, junk, _row((0, 0, 1), 0), junk, junk], [0] * 6, [0, 1, 3, 0, 2, 1], [0, 0], [0, 0], [nan, nan])
    assert o["rewards"].tolist() == [2.5, 0.0] and o["valid"].tolist() == [1, 1] and o["next_start"].tolist() == [0, 0]
    ro.tick([0, 0])
    assert ro.clock.tolist() == [1, 1]
    # step 1
    check([cmd(1, a0=1, a1=2, a2=3, a6=.5, a7=.5, a8=.5, a13=0.04), cmd(1, a0=10, a1=20, a2=30, a6=.5, a7=.5, a8=.5, a13=0.04)])
    o = step([_row((3, 4, 1), 1), junk, junk, _row((0, 0, 1), 0), junk, junk], [1, 0, 0, 0, 0, 0], [0] * 6, [0, 0], [0, 1], [nan, 3.0])
    assert o["rewards"].tolist() == [7.5, 1.5] and o["boot"].tolist() == [False, True] and o["next_start"].tolist() == [0, 1]
    assert o["ep_length"].tolist() == [0, 2]
    np.testing.assert_array_equal(o["ep_return"], [nan, 0.0])
    assert ag.wr_target[0].tolist() == [6, 8, 1]
    rows = start.copy()
    rows[:3] = nan
    ag.reset(rows, [0, 1])
    ro.tick([0, 1])
    assert ro.clock.tolist() == [2, 0] and ro.phase.tolist() == [[0, 1, 0, 0, 0, 0], [0] * 6, [0] * 6]
    # step 2: the clocks differ, env 1's scripted drone takes off again
    check([cmd(1, a0=4, a1=5, a2=6, a6=.5, a7=.5, a8=.5, a13=0.08), takeoff])
    o = step([_row((3, 4, 0.5), 1), junk, junk, _row((1.5, 2, 1), 0), junk, junk], [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0], [0, 0],
             [nan, nan])
    assert o["rewards"].tolist() == [-1.5, 2.5] and o["next_start"].tolist() == [1, 0] and o["ep_length"].tolist() == [3, 0]
    np.testing.assert_array_equal(o["ep_return"], [8.5, nan])
    ro.tick([0, 0])
    # step 3
    check([cmd(10, a0=0.12, a13=0.12), cmd(1, a0=10, a1=20, a2=30, a6=.5, a7=.5, a8=.5, a13=0.04)])
    o = step([junk, junk, junk, _row((3, 4, 1), 0), junk, junk], [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0], [0, 0], [nan, nan])
    assert o["rewards"].tolist() == [0.0, 2.5] and o["valid"].tolist() == [0, 1] and o["next_start"].tolist() == [1, 0]
    assert ag.alive.tolist() == [0, 1, 1, 1, 1, 1] and ag.run_length.tolist() == [3, 0, 0, 2, 0, 0]
    assert ag.wr_prev[[1, 2, 4, 5]].tolist() == [[0, 0, 1]] * 4
    ro.tick([0, 0])
    # past the table: LAND, then NONE
    check([cmd(5, a1=2.0, a13=2.0), cmd(1, a0=40, a1=50, a2=60, a6=.5, a7=.5, a8=.5, a13=0.08)])
    ro.tick(np.array([0, 0]))
    check([cmd(0), cmd(10, a0=0.12, a13=0.12)])
    assert ro.phase.tolist() == [[0, 1, 0, 0, 1, 0], [0, 1, 0, 0, 1, 0], [0, 1, 0, 0, 0, 0]] and ro.clock.tolist() == [5, 3]
    ro.tick(None)
    assert ro.clock.tolist() == [0, 0] and not ro.phase.any()
