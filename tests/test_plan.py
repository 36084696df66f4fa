"""The scripted racer's spline planner without a GPU (csrc/spline_plan.h, csrc/plan_host.cpp, include/adrp.h
adrp_race_plan, hardcoded.HardCodedCommander(planner=)).

* csrc/plan_host, the CPU build of the very header the kernel compiles, against scipy's splprep(s = 0.1) / splev
  at test time on the first 1,024 cases of the pinned sample (tests/plan_cases.py): the knot COUNT is equal in
  every case (a condition: FITPACK places the knots of one batch without refitting, and so must the planner), the
  knot values agree within 1e-14, the status flags are 0 (ier = 0, below the ceiling), coefficients and samples
  agree within ten times the largest difference measured over the whole 4,000-case sample
  (profiles/plan_parity.json: 3.6e-10, so 3.6e-9 here);
* the ctypes mirror of adrp_race_plan_io and every refusal of adrp_race_plan, reached without a device;
* the default planner="host" path is the one tests/golden/hardcoded_golden.npz pins, and the planner argument is
  checked and routed by HardCodedCommander, ControllerBank, simulate and tools/sim.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gym_pybullet_adrp_amd import _lib, sim
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander
from gym_pybullet_adrp_amd.utils import abi
from tests import plan_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 1024
PTR = 0x1000      # never dereferenced by a refusal
REQUIRED = ("obs", "samples", "ref", "status")
OPTIONAL = ("mask", "knots", "n_knots", "coef", "phase")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    start, gates = P.sample(CASES)
    return P.run_plan_host(start, gates, tmp_path_factory.mktemp("plan")), P.scipy_plan(start, gates)


# ---- plan_host against scipy ----------------------------------------------------------------------------------

def test_knot_count_equals_splprep(both):
    got, want = both
    assert np.array_equal(got["n"], want["n"]), np.flatnonzero(got["n"] != want["n"])[:10]
    assert set(want["n"].tolist()) == {15, 16}          # the sample has both counts: two lengths of the knot loop
    assert np.array_equal((got["status"] >> 8) & 255, want["n"])


def test_knot_values(both):
    got, want = both
    d = np.abs(got["t"] - want["t"]).max()
    print("knots: max abs difference", d)
    assert d <= P.KNOT_ATOL


def test_status_is_clean(both):
    got, _ = both
    assert not (got["status"] & (abi.PLAN_NOT_IER0 | abi.PLAN_CEILING)).any()
    it = (got["status"] >> 16) & 255
    assert (it >= 1).all() and (it <= 20).all()         # every case of the sample runs the p-iteration


def test_coefficients_and_samples(both):
    got, want = both
    dc, dr = np.abs(got["c"] - want["c"]).max(), np.abs(got["ref"] - want["ref"]).max()
    print("coefficients: max abs difference", dc, "samples:", dr, "bar", P.ATOL)
    assert dc <= P.ATOL and dr <= P.ATOL
    # x = 1 falls in the last non-empty interval: the curve ends on its last coefficient (three quotients of
    # equal lengths away from it: 1e-14 covers their rounding at |c| < 3)
    rows = np.arange(CASES)
    assert np.abs(got["ref"][:, -1] - got["c"][rows, :, got["n"] - 5]).max() <= 1e-14
    assert np.abs(got["ref"][:, 0] - got["c"][:, :, 0]).max() <= 1e-14


def test_plan_host_refuses_bad_files(tmp_path):
    import subprocess
    exe = P.build_plan_host()
    bad = tmp_path / "bad.f64"
    np.zeros(7).tofile(bad)
    ok = tmp_path / "ok.f64"
    np.linspace(0, 1, 5).tofile(ok)
    r = subprocess.run([exe, str(bad), str(ok), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "[cases][10]" in r.stderr
    assert subprocess.run([exe], capture_output=True).returncode == 2


# ---- the C-ABI without a device -------------------------------------------------------------------------------

def _header_fields(name):
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*(?:\[\w+\])?\s*;", body)


def test_struct_mirror_and_export(lib):
    """six 32-bit fields and nine pointers on LP64; the header, the mirror and the library agree"""
    assert ctypes.sizeof(abi.AdrpRacePlanIO) == 6 * 4 + 9 * 8
    assert _header_fields("adrp_race_plan_io") == [f[0] for f in abi.AdrpRacePlanIO._fields_]
    assert hasattr(lib, "adrp_race_plan")
    text = open(os.path.join(ROOT, "include", "adrp.h")).read()
    assert "#define ADRP_ABI_VERSION 2" in text           # purely additive: the ABI version stays
    for name, value in (("ADRP_PLAN_KNOTS", abi.PLAN_KNOTS), ("ADRP_PLAN_COEF", abi.PLAN_COEF),
                        ("ADRP_PLAN_OBS_MIN", abi.PLAN_OBS_MIN), ("ADRP_PLAN_NOT_IER0", abi.PLAN_NOT_IER0),
                        ("ADRP_PLAN_CEILING", abi.PLAN_CEILING)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert (abi.PLAN_KNOTS, abi.PLAN_COEF) == (P.NT, P.NC)


def _io(**change):
    io = abi.AdrpRacePlanIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRacePlanIO)
    io.num_envs, io.num_drones, io.ref_len, io.obs_stride = 4, 2, 300, 49
    for k in REQUIRED + OPTIONAL:
        setattr(io, k, PTR)
    for k, v in change.items():
        setattr(io, k, v)
    return io


REFUSALS = [(dict(struct_size=8), "struct_size"), (dict(num_envs=0), "num_envs"), (dict(num_envs=-3), "num_envs"),
            (dict(num_drones=0), "num_drones"), (dict(num_drones=abi.MAX_DRONES + 1), "num_drones"),
            (dict(ref_len=1), "ref_len"), (dict(ref_len=0), "ref_len"), (dict(obs_stride=27), "obs_stride"),
            (dict(obs_stride=0), "obs_stride")] + [({k: None}, "NULL buffer") for k in REQUIRED]


@pytest.mark.parametrize("change, word", REFUSALS)
def test_refusals(lib, change, word):
    """checked before any device call: they answer on a machine without a GPU"""
    io = _io(**change)
    assert lib.adrp_race_plan(ctypes.byref(io), None) == abi.ERR_INVALID
    msg = lib.adrp_last_error(None).decode()
    assert msg.startswith("adrp_race_plan:") and word in msg


def test_null_io_refused(lib):
    assert lib.adrp_race_plan(None, None) == abi.ERR_INVALID
    assert lib.adrp_last_error(None).decode() == "adrp_race_plan: io is NULL"


# ---- the Python surface ---------------------------------------------------------------------------------------

def test_default_planner_is_the_golden_host_path():
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "hardcoded_golden.npz"))
    obs0 = np.broadcast_to(G["hc_obs0"], (2, 2, G["hc_obs0"].shape[1])).copy()
    for kw in ({}, {"planner": "host"}):
        hc = HardCodedCommander(torch.from_numpy(obs0), **kw)
        assert hc.planner == "host" and hc.host_fallbacks == 0
        np.testing.assert_allclose(hc.reference_trajectory[1].numpy(), G["hc_ref"], rtol=0, atol=1e-12)


def test_planner_argument_checks(monkeypatch):
    obs = torch.zeros((1, 2, 49))
    with pytest.raises(ValueError, match="planner must be"):
        HardCodedCommander(obs, planner="gpu")
    with pytest.raises(ValueError, match="float32 tensor on a GPU"):
        HardCodedCommander(obs, planner="device")                 # a CPU tensor
    with pytest.raises(ValueError, match="float32 tensor on a GPU"):
        HardCodedCommander(obs.numpy(), planner="device")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="planner must be"):
        sim.simulate("level0", "hardcoded", n_runs=2, n_drones=2, planner="fpga")
    with pytest.raises(ValueError, match="planner must be"):
        sim.ControllerBank(None, ["hardcoded"], planner="fpga")
    with pytest.raises(_lib.AdrpError, match="no HIP device"):
        sim.simulate("level0", "hardcoded", n_runs=2, n_drones=2, planner="device")


def test_cli_routes_the_planner(monkeypatch):
    import types
    from tools import sim as cli
    seen = []
    fin = np.array([[4, 3]], np.int32)
    res = types.SimpleNamespace(finish_step=fin, elim_step=-np.ones((1, 2), np.int32), winner=sim.winner_of(fin),
                                finish_times=(fin - 1) / 25, episode_times=np.array([3 / 25]),
                                terminated=np.array([True]), truncated=np.array([False]))
    monkeypatch.setattr(cli, "simulate", lambda config, controller, **kw: seen.append(kw["planner"]) or res)
    cli.main(["--n_runs", "1", "--quiet"])
    cli.main(["--n_runs", "1", "--quiet", "--planner", "device"])
    assert seen == ["host", "device"]
    with pytest.raises(SystemExit):
        cli.main(["--planner", "fpga"])
