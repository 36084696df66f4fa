"""``adrp_race_roster_done`` (include/adrp_train.h, csrc/roster.hip) and ``RosterRolloutCollector(end_on=)``, the
part that needs no GPU: the entry point is declared and exported and the ABI version stays, every refusal is
reached without a device and names the function, and the numpy yardstick (tests/roster_end_on_reference.py) on
cases computed by hand."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from gym_pybullet_adrp_amd import _lib
from gym_pybullet_adrp_amd.rollout import RosterRolloutCollector
from gym_pybullet_adrp_amd.utils import abi
from tests.roster_end_on_reference import done_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUFFERS = ("clock", "phase", "ref", "offset", "setpoints", "learner_act", "codes", "args")
AGENT_BUFFERS = ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length")
PTR = 0x1000        # never dereferenced: every call below is refused before the first device call
L_, H_, P_, N_ = abi.ROSTER_LEARNER, abi.ROSTER_HARDCODED, abi.ROSTER_POLICY, abi.ROSTER_NONE


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_function(lib):
    text = open(os.path.join(ROOT, "include", "adrp_train.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src) if f.startswith("adrp_race_roster_")}
    assert declared == {"adrp_race_roster_done"} and hasattr(lib, "adrp_race_roster_done")
    assert "#define ADRP_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "adrp.h")).read()
    assert lib.adrp_abi_version() == 2


def _io(roles=(L_, H_, P_), index=None, **change):
    io = abi.AdrpRaceRosterIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceRosterIO)
    io.num_envs, io.num_drones, io.ref_len, io.ctrl_freq = 5, len(roles), 300, 25.0
    io.num_learners = sum(r == L_ for r in roles)
    learners = [n for n, r in enumerate(roles) if r == L_]
    for n, r in enumerate(roles):
        io.role[n] = r
        io.learner_index[n] = learners.index(n) if r == L_ else -1
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


def _refused(lib, io, agents, args, word):
    ref = None if io is None else ctypes.byref(io)
    ag = None if agents is None else ctypes.byref(agents)
    assert lib.adrp_race_roster_done(ref, ag, *args, None) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_race_roster_done:") and word in msg, msg


# adrp_race_roster_step's refusals of the roster (io, E / N / L, roles, learner_index)
@pytest.mark.parametrize("io, word", [
    (None, "io is NULL"), (_io(struct_size=8), "struct_size"),
    (_io(num_envs=0), "num_envs"), (_io(num_drones=0), "num_drones"), (_io(num_drones=abi.MAX_DRONES + 1), "num_drones"),
    (_io(num_learners=0), "num_learners"), (_io(num_learners=4), "num_learners"),
    (_io((L_, 4)), "role must be"), (_io((L_, H_), index={1: 0}), "learner_index must be -1"),
    (_io((L_, L_), index={1: 0}), "the same index"), (_io((L_, L_), index={1: 2}), "0..num_learners-1"),
    (_io((L_, N_, N_), num_learners=2), "not num_learners"),
])
def test_roster_refusals(lib, io, word):
    _refused(lib, io, _agents(num_drones=3 if io is None else io.num_drones), [PTR] * 3, word)


@pytest.mark.parametrize("change, word", [
    (None, "the agents io is NULL"), (dict(struct_size=8), "adrp_race_agents_io.struct_size"),
    (dict(num_envs=6), "differ from the roster's"), (dict(num_drones=2), "differ from the roster's"),
    (dict(obs_dim=48), "obs_dim"), (dict(num_gates=5), "num_gates"), (dict(alive=None), "NULL buffer"),
])
def test_agents_refusals(lib, change, word):
    _refused(lib, _io(), None if change is None else _agents(**change), [PTR] * 3, word)


@pytest.mark.parametrize("k", range(3))
def test_null_argument_refusals(lib, k):
    args = [PTR] * 3
    args[k] = None
    _refused(lib, _io(), _agents(), args, "NULL argument (term / trunc / mask_out)")


def test_collector_takes_end_on():
    """``end_on`` is an argument with the default "env"; a value other than the two is refused before anything else
    is looked at"""
    p = inspect.signature(RosterRolloutCollector.__init__).parameters
    assert p["end_on"].default == "env"
    for bad in ("learner", "drones", None, 1):
        with pytest.raises(ValueError, match="end_on must be 'env' or 'learners'"):
            RosterRolloutCollector(None, None, [], 4, end_on=bad)


def test_done_mask_by_hand():
    """3 envs x 3 drones, learners 0 and 2; drone 1's alive is never read (bytes that are not 0 / 1)"""
    alive = np.array([1, 7, 0,   0, 9, 0,   0, 0, 1], np.uint8)
    z = np.zeros(3, np.uint8)
    assert done_mask(alive, z, z, 3, [0, 2]).tolist() == [0, 1, 0]              # env 1: both learners dead
    assert done_mask(alive, [1, 0, 0], z, 3, [0, 2]).tolist() == [1, 1, 0]      # env 0 terminated
    assert done_mask(alive, z, [0, 0, 1], 3, [0, 2]).tolist() == [0, 1, 1]      # env 2 truncated
    assert done_mask(alive, z, z, 3, [1]).tolist() == [0, 0, 1]                 # one learner, drone 1: any non-zero byte is alive
    assert done_mask(alive, z, z, 3, [0]).tolist() == [0, 1, 1]
    out = done_mask(alive, [1, 1, 1], [1, 1, 1], 3, [0, 1, 2])
    assert out.dtype == np.uint8 and out.tolist() == [1, 1, 1]
