"""C-ABI surface of the per-drone race agents (include/adrp.h adrp_race_agents_*, csrc/agents.hip), the part
that needs no GPU: the header / library / ctypes mirror agree, every refusal is reached without a device and
names the function and its cause, the numpy yardstick (tests/agents_reference.py) on a case computed by hand and
its reward against the oracle's RewardWrapper, and PPOLearner.train's refusals on a collector with ``valid``.

Two refusals of adrp_race_agents_step_env need a handle to refuse, a non-race one and a race one of another shape;
creating a handle needs a device, so they are in tests/test_agents_gpu.py
(test_env_entry_reads_the_handle_image_and_refuses_other_handles), which also checks that the refused calls leave
the agents' state untouched.  The NULL handle is refused here."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_pybullet_adrp_amd import _lib
from gym_pybullet_adrp_amd.utils import abi
from tests import agents_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGENTS_FUNCTIONS = {"adrp_race_agents_reset", "adrp_race_agents_step", "adrp_race_agents_step_env"}
BUFFERS = ("wr_gate", "wr_target", "wr_prev", "alive", "run_return", "run_length")
PTR = 0x1000        # never dereferenced: every call below is refused before the first device call


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_agents_functions(lib):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src) if f.startswith("adrp_race_agents_")}
    assert declared == AGENTS_FUNCTIONS
    assert not [f for f in declared if not hasattr(lib, f)]
    assert "#define ADRP_ABI_VERSION 2" in text           # purely additive: the ABI version stays
    assert f"#define ADRP_AGENTS_OBS_MIN {abi.AGENTS_OBS_MIN}" in text


def _io(**change):
    io = abi.AdrpRaceAgentsIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceAgentsIO)
    io.num_envs, io.num_drones, io.obs_dim, io.num_gates = 5, 2, 55, 4
    for k in BUFFERS:
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


def test_struct_mirror():
    """the header's struct on LP64: six 32-bit fields, six pointers"""
    assert ctypes.sizeof(abi.AdrpRaceAgentsIO) == 6 * 4 + 6 * 8
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    body = re.search(r"typedef struct adrp_race_agents_io \{(.*?)\} adrp_race_agents_io;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in abi.AdrpRaceAgentsIO._fields_]
    assert [f[0] for f in abi.AdrpRaceAgentsIO._fields_][6:] == list(BUFFERS)


def _calls(lib, io):
    ref = None if io is None else ctypes.byref(io)
    return (("adrp_race_agents_reset", lambda: lib.adrp_race_agents_reset(ref, PTR, PTR, None)),
            ("adrp_race_agents_step", lambda: lib.adrp_race_agents_step(ref, *[PTR] * 6, 0.99, *[PTR] * 5, None)),
            ("adrp_race_agents_step_env", lambda: lib.adrp_race_agents_step_env(ref, PTR, *[PTR] * 4, 0.99, *[PTR] * 5, None)))


REFUSALS = [(dict(struct_size=8), "struct_size"), (dict(struct_size=ctypes.sizeof(abi.AdrpRaceAgentsIO) + 8), "struct_size"),
            (dict(num_envs=0), "num_envs"), (dict(num_envs=-2), "num_envs"),
            (dict(num_drones=0), "num_drones"), (dict(num_drones=abi.MAX_DRONES + 1), "num_drones"),
            (dict(obs_dim=48), "obs_dim"), (dict(num_gates=-1), "num_gates"), (dict(num_gates=5), "num_gates"),
            (dict(num_envs=2 ** 31 - 1, num_drones=8), "too large")] + [({k: None}, "NULL buffer") for k in BUFFERS]


@pytest.mark.parametrize("change, word", REFUSALS)
def test_io_refusals(lib, change, word):
    """checked before any device call (and before the handle is looked at): they answer without a GPU"""
    io = _io(**change)
    for fn, call in _calls(lib, io):
        assert call() == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith(fn + ":") and word in msg


def test_null_refusals(lib):
    for fn, call in _calls(lib, None):
        assert call() == abi.ERR_INVALID
        assert lib.adrp_last_error(None).decode() == f"{fn}: io is NULL"
    io = _io()
    ref = ctypes.byref(io)
    assert lib.adrp_race_agents_reset(ref, None, PTR, None) == abi.ERR_INVALID          # (a NULL mask is every env)
    assert lib.adrp_last_error(None).decode() == "adrp_race_agents_reset: NULL argument (obs)"
    for k in range(11):
        args = [PTR] * 11
        args[k] = None
        assert lib.adrp_race_agents_step(ref, *args[:6], 0.99, *args[6:], None) == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith("adrp_race_agents_step:") and "NULL" in msg
        assert ("obs / gate / flags / term / trunc / boot_value" if k < 6 else
                "rewards / valid / next_start / ep_return / ep_length") in msg
    assert lib.adrp_race_agents_step_env(ref, None, *[PTR] * 4, 0.99, *[PTR] * 5, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_agents_step_env: the handle is NULL"


def _row(pos, gate, D=49):
    """an obs row: the position, the four gates at (3,4,1) (6,8,1) (0,0,1) (0,0,1), the gate id in column 48"""
    row = np.zeros(D, np.float32)
    row[0:3] = pos
    row[12:28] = [3, 4, 1, 0, 6, 8, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    row[48] = gate
    return row


def test_reference_by_hand():
    """2 envs x 2 drones (slots 0, 1 | 2, 3), gamma 0.5, every drone reset at (0, 0, 1) with gate 0: target (3, 4, 1).
    step 0  slot 0 flies to (1.5, 2, 1): xy distance 5 -> 2.5, reward 2.5.
            slot 1 drops to (0, 0, 0.5) and is eliminated: z term 0 - 0.5, r_col -1: reward -1.5; its agent
            episode ends (return -1.5, length 1) while env 0 goes on.
            slot 2 reaches (3, 4, 1) and passes gate 0: the target becomes gate 1 at (6, 8, 1) before the
            distances are taken, 10 -> 5, r_passed 5: reward 10.
            slot 3 stays: reward 0.
    step 1  slot 0 reaches (3, 4, 1.25) with gate 4 = num_gates and finishes: 2.5 - 0.25 + 5 + 10 = 17.25, the
            target stays; episode return 19.75, length 2.  Env 0 terminates (both drones done).
            slot 1 is dead: its row is NaN, reward 0, not valid, start 1.
            env 1 is truncated: slot 2 stays, raw 0, stored 0 + 0.5 * 3 = 1.5, episode 10 over 2 steps;
            slot 3 flies to (0.75, 1, 1): 5 -> 3.75, raw 1.25, stored 1.25 + 0.5 * -2 = 0.25.
            Both envs are reset by the mask.
    step 2  slot 0 rises to (0, 0, 1.5): -0.5.  slot 1 (alive again) reaches (3, 4, 1) without a gate: 5.
            slot 2 stays: 0.  slot 3 flies to (1.5, 2, 1) and carries both flags: 2.5 + 10, no r_col."""
    nan = np.nan
    ag = R.Agents(2, 2, 49, 4)
    start = np.stack([_row((0, 0, 1), 0)] * 4)
    ag.reset(start)
    assert ag.alive.tolist() == [1] * 4 and ag.wr_target.tolist() == [[3, 4, 1]] * 4 and ag.wr_prev.tolist() == [[0, 0, 1]] * 4
    o = ag.step(np.stack([_row((1.5, 2, 1), 0), _row((0, 0, 0.5), 0), _row((3, 4, 1), 1), _row((0, 0, 1), 0)]),
                [0, 0, 1, 0], [0, 1, 0, 0], [0, 0], [0, 0], [nan] * 4, 0.5)
    assert o["rewards"].tolist() == [2.5, -1.5, 10.0, 0.0] and o["valid"].tolist() == [1, 1, 1, 1]
    assert o["next_start"].tolist() == [0, 1, 0, 0] and o["ep_length"].tolist() == [0, 1, 0, 0]
    np.testing.assert_array_equal(o["ep_return"], [nan, -1.5, nan, nan])
    assert ag.alive.tolist() == [1, 0, 1, 1] and ag.wr_gate.tolist() == [0, 0, 1, 0] and ag.wr_target[2].tolist() == [6, 8, 1]
    o = ag.step(np.stack([_row((3, 4, 1.25), 4), np.full(49, nan, np.float32), _row((3, 4, 1), 1), _row((0.75, 1, 1), 0)]),
                [4, 0, 1, 0], [2, 1, 0, 0], [1, 0], [0, 1], [nan, nan, 3.0, -2.0], 0.5)
    assert o["rewards"].tolist() == [17.25, 0.0, 1.5, 0.25] and o["valid"].tolist() == [1, 0, 1, 1]
    assert o["next_start"].tolist() == [1, 1, 1, 1] and o["ep_length"].tolist() == [2, 0, 2, 2]
    np.testing.assert_array_equal(o["ep_return"], [19.75, nan, 10.0, 1.25])
    assert o["boot"].tolist() == [False, False, True, True]
    assert ag.wr_gate.tolist() == [4, 0, 1, 0] and ag.wr_target[0].tolist() == [3, 4, 1] and ag.alive.tolist() == [0, 0, 1, 1]
    ag.reset(start, [1, 1])
    assert ag.alive.tolist() == [1] * 4 and ag.run_length.tolist() == [0] * 4 and ag.wr_gate.tolist() == [0] * 4
    o = ag.step(np.stack([_row((0, 0, 1.5), 0), _row((3, 4, 1), 0), _row((0, 0, 1), 0), _row((1.5, 2, 1), 0)]),
                [0, 0, 0, 0], [0, 0, 0, 3], [0, 0], [0, 0], [nan] * 4, 0.5)
    assert o["rewards"].tolist() == [-0.5, 5.0, 0.0, 12.5] and o["valid"].tolist() == [1] * 4
    assert o["next_start"].tolist() == [0, 0, 0, 1] and o["ep_length"].tolist() == [0, 0, 0, 1]
    np.testing.assert_array_equal(o["ep_return"], [nan, nan, nan, 12.5])
    # a masked reset leaves the other env alone, NaN rows included
    rows = start.copy()
    rows[2:] = nan
    ag.reset(rows, [1, 0])
    assert ag.run_length.tolist() == [0, 0, 1, 1] and ag.alive.tolist() == [1, 1, 1, 0]


def test_reference_reward_is_the_oracles():
    """the restatement's raw reward on drone rows against the unchanged, reference-pinned oracle
    (oracle.RewardWrapperState.step(row, became_done, finished)), slot by slot over constructed sequences; the
    oracle reads the gate id in column 48, which the sequences keep equal to the gate input"""
    from oracle import oracle as O
    E, N, D = 7, 3, 55
    first, steps = R.sequence(E, N, D, num_gates=4, T=6, seed=5)
    ag = R.Agents(E, N, D, 4)
    ag.reset(first)
    orc = [O.RewardWrapperState(first[j]) for j in range(E * N)]
    compared = 0
    for s in steps:
        alive = ag.alive.copy()
        o = ag.step(s["obs"], s["gate"], s["flags"], s["term"], s["trunc"], s["boot_value"], 0.99)
        for j in np.nonzero(alive)[0]:
            became_done, finished = (s["flags"][j] & 3) != 0, (s["flags"][j] & 2) != 0
            want = orc[j].step(s["obs"][j], became_done, finished)
            assert abs(o["raw"][j] - want) <= 1e-12 * max(1.0, abs(want))
            assert orc[j].gate.value == ag.wr_gate[j]
            np.testing.assert_array_equal(orc[j].target, ag.wr_target[j])
            compared += 1
        ag.reset(s["reset_obs"], s["mask"])
        for j in np.nonzero(np.repeat(s["mask"] != 0, N))[0]:
            orc[j] = O.RewardWrapperState(s["reset_obs"][j])
    assert compared > 60


def test_sequences_hold_what_the_gpu_tests_need():
    """the constructed streams cannot pass vacuously: each kind of slot occurs"""
    for E, N, G in ((70, 3, 4), (9, 8, 2), (90, 3, 4)):
        first, steps = R.sequence(E, N, 49, num_gates=G, T=6, seed=1)
        ag = R.Agents(E, N, 49, G)
        ag.reset(first)
        seen = dict(passed=0, finished=0, both=0, elim_on_trunc=0, dead=0, boot=0, reset=0)
        for s in steps:
            alive = ag.alive != 0
            before = ag.wr_gate.copy()
            o = ag.step(s["obs"], s["gate"], s["flags"], s["term"], s["trunc"], s["boot_value"], 0.9)
            seen["passed"] += int((alive & (ag.wr_gate > before)).sum())
            seen["finished"] += int((alive & (s["gate"] == G) & ((s["flags"] & 2) != 0)).sum())
            seen["both"] += int((alive & (s["flags"] == 3)).sum())
            seen["elim_on_trunc"] += int((alive & ((s["flags"] & 1) != 0) & np.repeat(s["trunc"] != 0, N)).sum())
            seen["dead"] += int((~alive & np.isnan(s["obs"][:, 0])).sum())
            seen["boot"] += int(o["boot"].sum())
            seen["reset"] += int(s["mask"].sum())
            assert np.isfinite(o["rewards"]).all() and (o["rewards"][~alive] == 0).all()
            ag.reset(s["reset_obs"], s["mask"])
        assert all(v > 0 for v in seen.values()), seen


class _Col:
    """what PPOLearner.train reads of a collector"""


def test_train_refuses_wrong_valid_permutations(monkeypatch):
    """the [n_epochs, n_valid] shape and the indices of invalid rows are refused before any update (host logic:
    the learner is built without a device handle)"""
    import torch

    from gym_pybullet_adrp_amd.ppo import PPOLearner
    ln = PPOLearner.__new__(PPOLearner)
    ln.n_epochs, ln.batch_size, ln.device, ln.h = 2, 4, torch.device("cpu"), None
    called = []
    ln.update = lambda *a, **k: called.append(a[-1].tolist())
    col = _Col()
    col.T, col.E = 3, 2
    col.obs, col.actions = torch.zeros(3, 2, 5), torch.zeros(3, 2, 4)
    col.values = col.log_probs = col.advantages = col.returns = torch.zeros(3, 2)
    col.valid = torch.tensor([[1, 0], [1, 1], [0, 1]], dtype=torch.uint8)       # valid flat rows 0, 2, 3, 5
    with pytest.raises(ValueError, match="n_valid = 4"):
        ln.train(col, torch.zeros((2, 6), dtype=torch.int64))
    with pytest.raises(ValueError, match="invalid row"):
        ln.train(col, torch.tensor([[0, 2, 3, 5], [5, 3, 1, 0]]))
    with pytest.raises(ValueError, match="invalid row"):
        ln.train(col, torch.tensor([[0, 2, 3, 5], [5, 3, 6, 0]]))
    assert called == []
    col.valid = torch.zeros((3, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="no valid sample"):
        ln.train(col)
