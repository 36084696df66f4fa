"""The scripted racer's spline planner on the device (csrc/plan_kernel.h, include/adrp.h adrp_race_plan,
HardCodedCommander(planner="device")).  Needs an MI355X: -m gpu.

Inputs are the pinned sample of tests/plan_cases.py written into observation rows.  The yardsticks are
``hardcoded.plan`` (scipy splprep / splev, what planner="host" runs) on the same rows and csrc/plan_host, the CPU
build of the header the kernel compiles.  Knot counts must be equal, knot values within 1e-14, the status flags
0; coefficients and samples within ten times the largest plan_host-to-scipy difference measured over the whole
sample (tests/plan_cases.py ATOL, 3.6e-9 m; profiles/plan_parity.json).  Race outcomes are not asserted: a 1e-10 m
setpoint difference is allowed to move a finish step."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.commands import CMD_ARGS  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander, plan  # noqa: E402
from gym_pybullet_adrp_amd.sim import ControllerBank, simulate  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from tests import plan_cases as P  # noqa: E402
from tests.test_sim_gpu import reset_obs, stub_env  # noqa: E402

SHAPES = [(1, 1), (3, 2), (13, 5), (70, 3)]      # (13, 5) is 65 lanes: one past a wave; (70, 3) is 210: a partial last wave
FLAGS = abi.PLAN_NOT_IER0 | abi.PLAN_CEILING
SENTINEL = -77.25


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """the first 210 cases of the sample, planned once by scipy (hardcoded.plan) and by plan_host"""
    count = max(E * N for E, N in SHAPES)
    start, gates = P.sample(count)
    host = np.stack([plan(start[i], gates[i]) for i in range(count)])
    return start, gates, host, P.scipy_plan(start, gates), P.run_plan_host(start, gates, tmp_path_factory.mktemp("plan"))


def device_plan(obs, E, N, mask=None, ref=None, phase=None, stride=None):
    """adrp_race_plan on obs rows (a float32 cuda tensor) with every optional output"""
    lib, dev = _lib.load(), obs.device
    out = {"ref": torch.full((E, N, P.L, 3), SENTINEL, dtype=torch.float64, device=dev) if ref is None else ref,
           "status": torch.full((E, N), -1, dtype=torch.int32, device=dev),
           "knots": torch.full((E, N, abi.PLAN_KNOTS), SENTINEL, dtype=torch.float64, device=dev),
           "n_knots": torch.full((E, N), -1, dtype=torch.int32, device=dev),
           "coef": torch.full((E, N, 3, abi.PLAN_COEF), SENTINEL, dtype=torch.float64, device=dev)}
    samples = torch.as_tensor(np.linspace(0, 1, P.L), device=dev)
    io = abi.AdrpRacePlanIO()
    io.struct_size = ctypes.sizeof(abi.AdrpRacePlanIO)
    io.num_envs, io.num_drones, io.ref_len = E, N, P.L
    io.obs_stride = obs.shape[-1] if stride is None else stride
    io.obs, io.samples = obs.data_ptr(), samples.data_ptr()
    io.mask = None if mask is None else mask.data_ptr()
    io.phase = None if phase is None else phase.data_ptr()
    for k, v in out.items():
        setattr(io, k, v.data_ptr())
    rc = lib.adrp_race_plan(ctypes.byref(io), _lib._raw_stream(dev.index))
    assert rc == 0, lib.adrp_last_error(None).decode()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_against(got, host, sci, ph, E, N):
    """device outputs [E, N, ...] against scipy (host: hardcoded.plan's samples, sci: knots and coefficients) and
    plan_host, on the first E * N cases"""
    C = E * N
    flat = {k: v.reshape((C,) + v.shape[2:]) for k, v in got.items()}
    assert not (flat["status"] & FLAGS).any()
    assert np.array_equal(flat["n_knots"], sci["n"][:C]) and np.array_equal((flat["status"] >> 8) & 255, sci["n"][:C])
    assert np.array_equal(flat["status"], ph["status"][:C])                  # flags, knot count, p-iterations
    dk = np.abs(flat["knots"] - sci["t"][:C]).max()
    dr, dc = np.abs(flat["ref"] - host[:C]).max(), np.abs(flat["coef"] - sci["c"][:C]).max()
    pk, pr, pc = (np.abs(flat[a] - ph[b][:C]).max() for a, b in (("knots", "t"), ("ref", "ref"), ("coef", "c")))
    print(f"E={E} N={N}: vs scipy knots {dk:.3g} ref {dr:.3g} coef {dc:.3g}; vs plan_host knots {pk:.3g} ref {pr:.3g} coef {pc:.3g}")
    assert dk <= P.KNOT_ATOL and pk <= P.KNOT_ATOL
    assert dr <= P.ATOL and dc <= P.ATOL
    assert pr <= P.ATOL and pc <= P.ATOL


@pytest.mark.parametrize("E, N", SHAPES)
def test_device_plan_equals_scipy_and_plan_host(cases, E, N):
    start, gates, host, sci, ph = cases
    C = E * N
    obs = torch.from_numpy(P.obs_rows(start[:C], gates[:C])).cuda()
    check_against(device_plan(obs, E, N), host, sci, ph, E, N)


def test_strided_compete_rows(cases):
    """COMPETE rows with N = 3 are 49 + 12 floats wide: the planner reads its 28 in place, whatever the rest holds"""
    start, gates, host, sci, ph = cases
    E, N, D = 4, 3, 49 + 6 * 2
    obs = torch.from_numpy(P.obs_rows(start[:E * N], gates[:E * N], width=D, fill=1e6)).cuda()
    check_against(device_plan(obs, E, N), host, sci, ph, E, N)
    hc = HardCodedCommander(obs.reshape(E, N, D), planner="device")
    assert hc.host_fallbacks == 0 and np.abs(hc.reference_trajectory.cpu().numpy().reshape(E * N, P.L, 3) - host[:E * N]).max() <= P.ATOL
    # the drone-major slice of a wider buffer: rows 2 * D apart
    wide = torch.full((E * N, 2 * D), 1e6, dtype=torch.float32, device="cuda")
    wide[:, :D] = obs
    got = device_plan(wide, E, N, stride=2 * D)
    assert np.abs(got["ref"].reshape(E * N, P.L, 3) - host[:E * N]).max() <= P.ATOL


def test_mask_leaves_the_other_envs_untouched(cases):
    start, gates, host, sci, ph = cases
    E, N = 13, 5
    obs = torch.from_numpy(P.obs_rows(start[:E * N], gates[:E * N])).cuda()
    mask = torch.zeros(E, dtype=torch.uint8, device="cuda")
    mask[[0, 5, 12]] = 1
    keep = ~mask.bool().cpu().numpy()
    ref = torch.randn((E, N, P.L, 3), dtype=torch.float64, device="cuda")
    before = ref.clone()
    phase = torch.ones((3, E, N), dtype=torch.uint8, device="cuda")
    got = device_plan(obs, E, N, mask=mask, ref=ref, phase=phase)
    assert torch.equal(ref[torch.from_numpy(keep).cuda()], before[torch.from_numpy(keep).cuda()])      # bit-identical
    assert (got["status"][keep] == -1).all() and (got["n_knots"][keep] == -1).all()
    assert (got["knots"][keep] == SENTINEL).all() and (got["coef"][keep] == SENTINEL).all()
    assert np.array_equal(phase.cpu().numpy(), np.broadcast_to(keep[None, :, None], (3, E, N)).astype(np.uint8))
    want = host[:E * N].reshape(E, N, P.L, 3)
    assert np.abs(got["ref"][~keep] - want[~keep]).max() <= P.ATOL and not (got["status"][~keep] & FLAGS).any()
    # the commander's replan(mask): planned envs restart, the others keep their trajectory and flags
    hc = HardCodedCommander(obs.reshape(E, N, 49), planner="device")
    for k in range(60):
        hc.predict(k / 25)
    traj, flags = hc.reference_trajectory.clone(), hc._flags.clone()
    assert bool(flags[0].all())
    hc.replan(obs.reshape(E, N, 49).flip(0).contiguous(), mask=mask)
    m = mask.bool()
    assert torch.equal(hc.reference_trajectory[~m], traj[~m]) and torch.equal(hc._flags[:, ~m], flags[:, ~m])
    assert not bool(hc._flags[:, m].any())
    assert np.abs(hc.reference_trajectory[m].cpu().numpy() - want[::-1][~keep]).max() <= P.ATOL
    assert (hc.plan_status[~m] == 0).all() and not bool((hc.plan_status[m] & FLAGS).any())


def test_status_exceptions(cases):
    """the two rare paths of HardCodedCommander: bit 0 re-plans that drone on the host, bit 1 raises plan()'s error"""
    start, gates, host, _, _ = cases
    E, N = 3, 2
    obs = torch.from_numpy(P.obs_rows(start[:E * N], gates[:E * N])).cuda().reshape(E, N, 49)
    hc = HardCodedCommander(obs, planner="device")
    assert hc.host_fallbacks == 0
    hc.reference_trajectory[1, 0] = SENTINEL
    hc.plan_status[1, 0] |= abi.PLAN_NOT_IER0
    hc._device_exceptions(obs)
    assert hc.host_fallbacks == 1
    assert np.array_equal(hc.reference_trajectory[1, 0].cpu().numpy(), host[2])          # scipy's own samples
    hc.plan_status[2, 1] |= abi.PLAN_CEILING
    with pytest.raises(ValueError, match="below the ceiling"):
        hc._device_exceptions(obs)
    # through the kernel: a NaN start gives NaN samples, which are not below the ceiling (plan()'s own test)
    bad = obs.clone()
    bad[0, 1, 0] = float("nan")
    with pytest.raises(ValueError, match="below the ceiling"):
        HardCodedCommander(bad, planner="device")


def test_controller_bank_flight_device_against_host():
    """ControllerBank.predict over a whole scripted flight: equal codes, args within the bar"""
    E, N, freq = 3, 2, 25
    obs = reset_obs("level0", E, N)
    a, b = ControllerBank(stub_env(E, N, obs.shape[2]), "hardcoded", planner="device"), ControllerBank(stub_env(E, N, obs.shape[2]), "hardcoded")
    a.reset(obs)
    b.reset(obs)
    assert a.commander.planner == "device" and b.commander.planner == "host" and a.commander.host_fallbacks == 0
    worst = 0.0
    for k in range((2 + N + 12 + 1) * freq + 1):
        ca, aa = a.predict(obs, k / freq)
        cb, ab = b.predict(obs, k / freq)
        assert aa.shape == (E, N, CMD_ARGS) and torch.equal(ca, cb), f"step {k}: codes"
        worst = max(worst, float((aa - ab).abs().max()))
    print("args: max abs difference over the flight", worst)
    assert worst <= P.ATOL
    assert torch.equal(a.phase, b.phase) and bool(a.phase.all())
    # a second wave re-plans in place
    a.reset(obs.flip(0).contiguous())
    b.reset(obs.flip(0).contiguous())
    assert float((a.commander.reference_trajectory - b.commander.reference_trajectory).abs().max()) <= P.ATOL


def test_simulate_with_the_device_planner():
    """two waves (3 + 2 runs); the times are finite, the outcomes themselves are not asserted"""
    times = simulate("level0", ["hardcoded"] * 2, n_runs=5, n_drones=2, num_envs=3, planner="device")
    print("episode times", times)
    assert len(times) == 5 and np.isfinite(times).all() and min(times) > 0
