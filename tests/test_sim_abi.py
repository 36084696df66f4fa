"""C-ABI surface of the batched race evaluation (include/adrp.h adrp_race_controllers / adrp_race_results_*,
csrc/sim.hip) and the host-side logic of gym_pybullet_adrp_amd/sim.py, the part that needs no GPU: the header /
library / ctypes mirrors agree, every refusal is reached without a device and names its cause, ``simulate``,
``ControllerBank`` and ``RaceResults`` refuse to run without a GPU, ``simulate``'s argument checks, and the numpy
yardstick (tests/sim_reference.py) on a case computed by hand."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from gym_pybullet_adrp_amd import _lib, sim
from gym_pybullet_adrp_amd.utils import abi
from tests import sim_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_FUNCTIONS = {"adrp_race_controllers", "adrp_race_results_begin", "adrp_race_results_step", "adrp_race_results_step_env"}
CTRL_BUFFERS = ("ref", "offset", "phase", "setpoints", "codes", "args")
RES_BUFFERS = ("open", "run_return", "run_length", "gates", "finish", "elim", "meta", "log_return", "log_length",
               "log_term", "log_trunc", "log_gates", "log_finish", "log_elim")
PTR = 0x1000      # never dereferenced by a refusal


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_and_library_exports_the_sim_functions(lib):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {f for f in re.findall(r"\b(adrp_[a-z_]+)\s*\(", src)
                if f.startswith("adrp_race_results_") or f == "adrp_race_controllers"}
    assert declared == SIM_FUNCTIONS
    assert not [f for f in declared if not hasattr(lib, f)]
    assert "#define ADRP_ABI_VERSION 2" in text           # purely additive: the ABI version stays


def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*(?:\[\w+\])?\s*;", body)


def test_struct_mirrors():
    """the header's structs on LP64: 4 + 8 32-bit fields and six pointers; six 32-bit fields and fourteen pointers"""
    assert ctypes.sizeof(abi.AdrpRaceCtrlIO) == 4 * 4 + 4 * abi.MAX_DRONES + 6 * 8
    assert ctypes.sizeof(abi.AdrpRaceResultsIO) == 6 * 4 + 14 * 8
    assert _header_fields("adrp_race_ctrl_io") == [f[0] for f in abi.AdrpRaceCtrlIO._fields_]
    assert _header_fields("adrp_race_results_io") == [f[0] for f in abi.AdrpRaceResultsIO._fields_]
    assert [f[0] for f in abi.AdrpRaceCtrlIO._fields_][-6:] == list(CTRL_BUFFERS)
    assert [f[0] for f in abi.AdrpRaceResultsIO._fields_][-14:] == list(RES_BUFFERS)
    assert (abi.RACE_CTRL_NONE, abi.RACE_CTRL_HARDCODED, abi.RACE_CTRL_POLICY) == (0, 1, 2)


def _ctrl(kinds=(1, 2), **change):
    io = abi.AdrpRaceCtrlIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceCtrlIO)
    io.num_envs, io.num_drones, io.ref_len = 4, len(kinds), 300
    for n, k in enumerate(kinds):
        io.kind[n] = k
    for k in CTRL_BUFFERS:
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


def _res(**change):
    io = abi.AdrpRaceResultsIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRaceResultsIO)
    io.num_envs, io.num_drones, io.capacity = 4, 2, 10
    for k in RES_BUFFERS:
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


CTRL_REFUSALS = [(dict(struct_size=8), "struct_size"), (dict(num_envs=0), "num_envs"), (dict(num_envs=-2), "num_envs"),
                 (dict(num_drones=0), "num_drones"), (dict(num_drones=abi.MAX_DRONES + 1), "num_drones"),
                 (dict(codes=None), "NULL buffer"), (dict(args=None), "NULL buffer"),
                 (dict(ref=None), "HARDCODED"), (dict(offset=None), "HARDCODED"), (dict(phase=None), "HARDCODED"),
                 (dict(ref_len=0), "HARDCODED"), (dict(setpoints=None), "POLICY")]


@pytest.mark.parametrize("change, word", CTRL_REFUSALS)
def test_controller_refusals(lib, change, word):
    """checked before any device call: they answer on a machine without a GPU"""
    io = _ctrl(**change)
    assert lib.adrp_race_controllers(ctypes.byref(io), 0.0, None) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_race_controllers") and word in msg


def test_controller_kind_and_null_refusals(lib):
    assert lib.adrp_race_controllers(None, 0.0, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_controllers: io is NULL"
    for bad in (3, -1):
        io = _ctrl(kinds=(0, bad))
        assert lib.adrp_race_controllers(ctypes.byref(io), 0.0, None) == abi.ERR_INVALID
        assert "kind" in lib.adrp_last_error(None).decode()


RES_REFUSALS = [(dict(struct_size=8), "struct_size"), (dict(num_envs=0), "num_envs"), (dict(num_drones=0), "num_drones"),
                (dict(num_drones=abi.MAX_DRONES + 1), "num_drones"), (dict(capacity=0), "capacity")] \
    + [({k: None}, "NULL buffer") for k in RES_BUFFERS]


@pytest.mark.parametrize("change, word", RES_REFUSALS)
def test_results_io_refusals(lib, change, word):
    io = _res(**change)
    calls = (("adrp_race_results_begin", lambda: lib.adrp_race_results_begin(ctypes.byref(io), 0, 2, None)),
             ("adrp_race_results_step", lambda: lib.adrp_race_results_step(ctypes.byref(io), PTR, PTR, PTR, PTR, PTR, None)),
             ("adrp_race_results_step_env", lambda: lib.adrp_race_results_step_env(ctypes.byref(io), PTR, PTR, PTR, PTR, None)))
    for fn, call in calls:
        assert call() == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith(fn + ":") and word in msg


def test_results_wave_and_null_refusals(lib):
    for fn, call in (("adrp_race_results_begin", lambda: lib.adrp_race_results_begin(None, 0, 1, None)),
                     ("adrp_race_results_step", lambda: lib.adrp_race_results_step(None, PTR, PTR, PTR, PTR, PTR, None)),
                     ("adrp_race_results_step_env", lambda: lib.adrp_race_results_step_env(None, PTR, PTR, PTR, PTR, None))):
        assert call() == abi.ERR_INVALID
        assert lib.adrp_last_error(None).decode() == fn + ": io is NULL"
    io = _res()
    for base, n_open, word in ((0, 5, "n_open"), (0, -1, "n_open"), (7, 4, "capacity"), (-1, 2, "capacity"), (10, 1, "capacity")):
        assert lib.adrp_race_results_begin(ctypes.byref(io), base, n_open, None) == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith("adrp_race_results_begin") and word in msg
        assert io.base == 0                                  # a refused begin leaves the io as it was
    for k in range(5):
        args = [PTR] * 5
        args[k] = None
        assert lib.adrp_race_results_step(ctypes.byref(io), *args, None) == abi.ERR_INVALID
        msg = lib.adrp_last_error(None).decode()
        assert msg.startswith("adrp_race_results_step:") and "NULL" in msg and "gate / flags / rew / term / trunc" in msg
    assert lib.adrp_race_results_step_env(ctypes.byref(io), None, PTR, PTR, PTR, None) == abi.ERR_INVALID
    assert "handle is NULL" in lib.adrp_last_error(None).decode()


def _stub_env():
    cfg = types.SimpleNamespace(autoreset=0, task=abi.TASK_RACE)
    return types.SimpleNamespace(cfg=cfg, NUM_DRONES=2, num_envs=3, CTRL_FREQ=25, device=torch.device("cuda", 0),
                                 h=types.SimpleNamespace(D=49))


def test_everything_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # (as tests/test_episode_abi.py: no skip with a GPU)
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        sim.RaceResults(3, 2, 5, 0)
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        sim.ControllerBank(_stub_env(), ["hardcoded", None])
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        sim.simulate("level0", ["hardcoded", "hardcoded"], n_runs=2, n_drones=2)


def test_simulate_argument_checks(monkeypatch):
    """refused before the device is looked for"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="controllers for 2 drones"):
        sim.simulate("level0", ["hardcoded"] * 3, n_runs=2, n_drones=2)
    with pytest.raises(ValueError, match="controllers for 3 drones"):
        sim.simulate("level0", ["hardcoded", None], n_runs=2, n_drones=3)
    with pytest.raises(ValueError, match="GUI"):
        sim.simulate("level0", "hardcoded", n_runs=2, n_drones=2, gui=True)
    with pytest.raises(ValueError, match="n_runs"):
        sim.simulate("level0", "hardcoded", n_runs=0, n_drones=2)
    with pytest.raises(ValueError, match="num_envs"):
        sim.simulate("level0", "hardcoded", n_runs=3, n_drones=2, num_envs=0)
    assert sim._expand("hardcoded", 3) == ["hardcoded"] * 3 and sim._expand([None], 2) == [None, None]


def test_reference_by_hand():
    """2 envs x 2 drones, 5 steps, runs 3 and 4 of a capacity of 6 (base 3).
    env 0: rewards 1, 0.5, 0.25, ...; drone 1 finishes at step 3 (flags 2), drone 0 finishes at step 4, which
           terminates the env: return 1 + 0.5 + 0.25 + 2 = 3.75 over 4 steps, gates [4, 4], finish [4, 3].
    env 1: drone 0 is eliminated at step 2 (flags 1); the env closes by truncation at step 3 with return
           -1 - 1 + 0.5 = -1.5 over 3 steps, gates [1, 2], elim [2, -1].
    step 5: both envs are closed: flags, gates, rewards and a second termination change nothing."""
    gate = [[[0, 1], [0, 0]], [[1, 2], [1, 1]], [[2, 4], [1, 2]], [[4, 4], [3, 3]], [[4, 4], [4, 4]]]
    flags = [[[0, 0], [0, 0]], [[0, 0], [1, 0]], [[0, 2], [1, 0]], [[2, 2], [1, 2]], [[3, 3], [3, 3]]]
    rew = [[1.0, -1.0], [0.5, -1.0], [0.25, 0.5], [2.0, 8.0], [16.0, 16.0]]
    term = [[0, 0], [0, 0], [0, 0], [1, 0], [1, 1]]
    trunc = [[0, 0], [0, 0], [0, 1], [0, 0], [0, 1]]
    acc = R.RaceAccounts(2, 2, 6)
    acc.begin(3, 2)
    left = []
    for t in range(5):
        acc.step(gate[t], flags[t], rew[t], term[t], trunc[t])
        left.append(acc.remaining)
    assert left == [2, 2, 1, 0, 0] and acc.logged == 2 and acc.steps == 5
    assert acc.log_return.tolist() == [0, 0, 0, 3.75, -1.5, 0] and acc.log_length.tolist() == [0, 0, 0, 4, 3, 0]
    assert acc.log_term.tolist() == [0, 0, 0, 1, 0, 0] and acc.log_trunc.tolist() == [0, 0, 0, 0, 1, 0]
    assert acc.log_gates[3:5].tolist() == [[4, 4], [1, 2]]
    assert acc.log_finish[3:5].tolist() == [[4, 3], [-1, -1]] and acc.log_elim[3:5].tolist() == [[-1, -1], [2, -1]]
    assert acc.log_finish[[0, 1, 2, 5]].tolist() == [[-1, -1]] * 4             # slots no run has written
    assert acc.episode_times(25)[3:5].tolist() == [3 / 25, 2 / 25]
    assert R.winner(acc.log_finish).tolist() == [-1, -1, -1, 1, -1, -1]
    assert sim.winner_of(acc.log_finish).tolist() == [-1, -1, -1, 1, -1, -1]
    assert R.winner([[5, 5, 7], [-1, 9, 9], [3, -1, 2]]).tolist() == [0, 1, 2]      # ties go to the lower index
    assert sim.winner_of(np.array([[5, 5, 7], [-1, 9, 9], [3, -1, 2]])).tolist() == [0, 1, 2]
    # a wave with one env open: env 1 never records
    acc.begin(0, 1)
    acc.step(gate[1], flags[1], rew[1], [0, 1], [0, 0])
    assert acc.remaining == 1 and acc.run_length.tolist() == [1, 0] and acc.run_elim.tolist() == [[-1, -1], [-1, -1]]
    # the POLICY command row: float32 setpoint widened, yaw in slot 9, the clock in slot 13, zeros elsewhere
    code, a = R.policy_command_row(np.array([0.1, -2.0, 0.75, 3.0], np.float32), 0.36)
    want = [0.0] * 14
    want[0], want[1], want[2], want[9], want[13] = float(np.float32(0.1)), -2.0, 0.75, 3.0, 0.36
    assert code == 1 and a.tolist() == want


def test_cli_table_and_arguments(monkeypatch, capsys):
    """tools/sim.py: the per-drone table from the result arrays, and the argument routing into simulate()"""
    from tools import sim as cli
    fin = np.array([[4, 3], [-1, -1], [9, 9], [-1, 7]], np.int32)
    res = types.SimpleNamespace(finish_step=fin, elim_step=np.array([[-1, -1], [2, 5], [-1, -1], [3, -1]], np.int32),
                                winner=sim.winner_of(fin), finish_times=np.where(fin >= 0, (fin - 1) / 25, np.nan),
                                episode_times=np.array([3, 4, 8, 6]) / 25, terminated=np.array([1, 1, 1, 0], bool),
                                truncated=np.array([0, 0, 0, 1], bool))
    rows = cli.table(res)
    assert rows[0] == (0, 0.5, pytest.approx((3 + 8) / 2 / 25, rel=1e-15), 0.5, 1)
    assert rows[1] == (1, 0.75, pytest.approx((2 + 8 + 6) / 3 / 25, rel=1e-15), 0.25, 2)
    seen = {}

    def fake(config, controller, **kw):
        seen.update(config=config, controller=controller, **kw)
        return res
    monkeypatch.setattr(cli, "simulate", fake)
    cli.main(["--config", "level1", "--controller", "hardcoded,zip:/x/y.zip,none", "--n_runs", "4", "--n_drones", "3", "--num_envs", "2"])
    assert seen["controller"] == ["hardcoded", "zip:/x/y.zip", None] and seen["config"] == "level1"
    assert (seen["n_runs"], seen["n_drones"], seen["num_envs"], seen["return_results"]) == (4, 3, 2, True)
    out = capsys.readouterr().out
    assert "episode times [s]: 0.12 0.16 0.32 0.24" in out and "(no finisher)" in out
