"""MultiHoverAviary HIP kernel (one lane per (env, drone), csrc/multihover_kernel.h).  Needs an MI355X: -m gpu.

References are assembled from what exists: the reference's own MultiHoverAviary episodes
(tests/golden/multihover_golden.npz), the unchanged single-drone CPU oracle, the oracle's force
assembly for the downwash, and HoverAviary's kernel for N = 1.

Bars (tests/test_hover_gpu.py): per state vector |x_gpu - x_ref| <= rtol * max(|x_ref|, floor), rtol 1e-9
(fp64) / 1e-4 (fp32), the floors of FLOORS; the action ring and the ints are exact.  Where both sides
are float32 roundings of float64 values (obs rows and rewards against the fixture), one float32 ulp
(2^-23) is added: values within the bar of each other may round to neighbouring float32s.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs import HoverAviary, MultiHoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import ActionType, Physics  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_hover_gpu import FLOORS, GROUPS, active_fields  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = {"fp64": 1e-9, "fp32": 1e-4}
F32_ULP = 2.0 ** -23
UNCOUPLED = [Physics.PYB, Physics.DYN, Physics.PYB_GND, Physics.PYB_DRAG]
DOWNWASH = [Physics.PYB_DW, Physics.PYB_GND_DRAG_DW]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "multihover_golden.npz"))


def real_of(env):
    return np.float64 if env.cfg.precision else np.float32


def field_index(env):
    names, inames = env.state_field_names()
    return {n: k for k, n in enumerate(names)}, {n: k for k, n in enumerate(inames)}, names


def put_state(env, f, i):
    real = real_of(env)
    env.set_state(torch.from_numpy(f.astype(real)), torch.from_numpy(i.astype(np.int32)))


def get_state(env):
    f, i = env.get_state()
    return f.double().cpu().numpy(), i.cpu().numpy()


def random_multi_state(rng, env, spread=0.3, tilt=0.25, vel=0.5, omega=2.0):
    """random airborne states about the drones' targets, [nf, E*N] float64 (representable in the env's
    precision) and ints replicated per env"""
    E, N = env.num_envs, env.NUM_DRONES
    idx, iidx, names = field_index(env)
    f = np.zeros((len(names), E * N))
    i = np.zeros((3, E * N), np.int32)
    center = np.tile(env.TARGET_POS, (E, 1))                     # column e*N + n
    pos = center + rng.uniform(-spread, spread, (E * N, 3))
    pos[:, 2] = np.maximum(pos[:, 2], 0.25)
    rpy = rng.uniform(-tilt, tilt, (E * N, 3)) * np.array([1, 1, 4])
    q = np.array([O.quat_from_euler(r) for r in rpy])
    lag = np.array([O.quat_from_euler(r + rng.uniform(-0.01, 0.01, 3)) for r in rpy])
    v = rng.uniform(-vel, vel, (E * N, 3))
    w = rng.uniform(-omega, omega, (E * N, 3))
    for k, ax in enumerate("xyz"):
        f[idx[f"pos_{ax}"]] = pos[:, k]; f[idx[f"vel_{ax}"]] = v[:, k]
        f[idx[f"omega_{ax}"]] = w[:, k]; f[idx[f"angv_{ax}"]] = w[:, k]
    for k, ax in enumerate("xyzw"):
        f[idx[f"quat_{ax}"]] = q[:, k]; f[idx[f"link_quat_{ax}"]] = lag[:, k]
    for k in range(4):
        f[idx[f"last_rpm_{k}"]] = rng.uniform(0.8, 1.2, E * N) * 16364.0
    ring = [k for k, n in enumerate(names) if n.startswith("ring_")]
    f[ring] = rng.uniform(-1, 1, (len(ring), E * N))
    S = env.PYB_STEPS_PER_CTRL
    i[iidx["step_counter"]] = np.repeat(rng.integers(0, 200, E) * S, N)
    i[iidx["ring_head"]] = np.repeat(rng.integers(0, env.ACTION_BUFFER_SIZE, E), N)
    i[iidx["episode"]] = np.repeat(rng.integers(1, 5, E), N)
    f = f.astype(real_of(env)).astype(np.float64)
    return f, i


def hover_oracle(env, n):
    """the unchanged single-drone oracle standing in for drone n of every env: HoverAviary at the drone's
    initial position with the drone's target, no auto-reset"""
    cfg = _lib.default_config(abi.TASK_HOVER)
    src = env.cfg
    for k in ("physics", "act_type", "num_envs", "pyb_freq", "ctrl_freq", "action_buffer_size", "precision",
              "link_frame_lag", "seed"):
        setattr(cfg, k, getattr(src, k))
    cfg.autoreset = 0
    abi.set_vec(cfg.init_xyz[0], env.INIT_XYZS[n])
    abi.set_vec(cfg.target_pos, env.TARGET_POS[n])
    return O.Oracle(cfg)


def group_err(fg, fo, idx, g):
    rows = [idx[n] for n in GROUPS[g]]
    d = np.linalg.norm(fg[rows] - fo[rows], axis=0)
    return d / np.maximum(np.linalg.norm(fo[rows], axis=0), FLOORS[g])


def assert_state_close(fg, fo, idx, names, rtol, active, what=""):
    for k, nme in enumerate(names):
        if nme.startswith("ring_"):
            np.testing.assert_array_equal(fg[k], fo[k], err_msg=nme)
    for g in sorted(active):
        err = group_err(fg, fo, idx, g)
        assert err.max() <= rtol, f"{what}{g}: max rel err {err.max():.3e} (column {err.argmax()})"


def assert_rows_close(og, oo, rtol, what=""):
    """obs rows [..., 12+]: pos, rpy, vel, ang_v vectors at the bar; the action history exact"""
    np.testing.assert_array_equal(og[..., 12:], oo[..., 12:], err_msg=what + "ring")
    for nm, sl in (("pos", slice(0, 3)), ("rpy", slice(3, 6)), ("vel", slice(6, 9)), ("ang_v", slice(9, 12))):
        d = np.linalg.norm(og[..., sl].astype(np.float64) - oo[..., sl], axis=-1)
        err = d / np.maximum(np.linalg.norm(oo[..., sl].astype(np.float64), axis=-1), 1e-3)
        assert err.max() <= rtol, f"{what}obs {nm}: max rel err {err.max():.3e}"


def trunc_mismatches_at_threshold(tr_g, tr_ref, kin_ref, bar):
    """MultiHoverAviary.py:112-130 (|x|, |y| > 2, z > 2, |roll|, |pitch| > 0.4 of any drone): the flag may
    differ only for an env where a drone of the reference end state kin_ref [E, N, >=5] (pos, roll, pitch)
    sits within the bar of one of these thresholds, relative to the threshold"""
    bad = np.flatnonzero(tr_g != tr_ref)
    for e in bad:
        x = kin_ref[e].astype(np.float64)
        margin = min(np.abs(np.abs(x[:, 0]) - 2.0).min() / 2.0, np.abs(np.abs(x[:, 1]) - 2.0).min() / 2.0,
                     np.abs(x[:, 2] - 2.0).min() / 2.0, np.abs(np.abs(x[:, 3]) - 0.4).min() / 0.4,
                     np.abs(np.abs(x[:, 4]) - 0.4).min() / 0.4)
        assert margin <= bar, f"env {e}: truncated gpu {tr_g[e]} ref {tr_ref[e]}, {margin:.2e} from the nearest threshold"
    return len(bad)


def flags_numpy(kin, target, counter=None, trunc_steps=1921):
    """terminated / truncated of MultiHoverAviary.py:92-130 from end states kin [E, N, >=5] (pos, roll, pitch)"""
    dist = np.zeros(kin.shape[0])
    for n in range(kin.shape[1]):
        dist = dist + np.linalg.norm(target[n] - kin[:, n, :3].astype(np.float64), axis=-1)
    out = (np.abs(kin[..., 0]) > 2.0) | (np.abs(kin[..., 1]) > 2.0) | (kin[..., 2] > 2.0) | \
          (np.abs(kin[..., 3]) > 0.4) | (np.abs(kin[..., 4]) > 0.4)
    tr = out.any(axis=1)
    if counter is not None:
        tr = tr | (counter >= trunc_steps)
    return dist < 1e-4, tr


# ---------------------------------------------------------------------------------------------
# C1  golden replay: the reference's own MultiHoverAviary(DYN) episodes, teacher-forced
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("case,N,act", [("rpm2", 2, ActionType.RPM), ("rpm3", 3, ActionType.RPM),
                                        ("one2", 2, ActionType.ONE_D_RPM)])
def test_golden_replay(fx, case, N, act, precision):
    rtol = RTOL[precision]
    init, ring0, acts = fx[f"{case}_init"], fx[f"{case}_ring0"], fx[f"{case}_act"]
    E, T, A, B = acts.shape[0], acts.shape[1], acts.shape[3], ring0.shape[1]
    env = MultiHoverAviary(num_drones=N, physics=Physics.DYN, act=act, num_envs=E, precision=precision, autoreset=False)
    np.testing.assert_array_equal(env.TARGET_POS, fx[f"{case}_target"])
    idx, iidx, names = field_index(env)
    ref_state = fx[f"{case}_state"]           # [E, T, N, 16] pos, quat, vel, rpy_rates, ang_v
    for t in range(T):
        st = (np.concatenate([init, np.zeros((E, N, 3))], -1) if t == 0 else ref_state[:, t - 1]).reshape(E * N, 16)
        f = np.zeros((len(names), E * N))
        for k, ax in enumerate("xyz"):
            f[idx[f"pos_{ax}"]] = st[:, k]; f[idx[f"vel_{ax}"]] = st[:, 7 + k]
            f[idx[f"omega_{ax}"]] = st[:, 10 + k]; f[idx[f"angv_{ax}"]] = st[:, 13 + k]
        for k, ax in enumerate("xyzw"):
            f[idx[f"quat_{ax}"]] = st[:, 3 + k]; f[idx[f"link_quat_{ax}"]] = st[:, 3 + k]
        hist = np.concatenate([ring0, acts[:, :t]], axis=1)[:, t:t + B]   # the last B entries [E, B, N, A], oldest first
        for s in range(B):
            for j in range(A):
                f[idx[f"ring_{s}_{j}"]] = hist[:, s, :, j].reshape(E * N)
        i = np.zeros((3, E * N), np.int32)
        i[iidx["step_counter"]] = 8 * t
        put_state(env, f, i)                   # ring_head 0: slot s is the s-th oldest entry
        obs, rew, te, tr, _ = env.step(torch.from_numpy(acts[:, t]))
        torch.cuda.synchronize()
        og = obs.cpu().numpy()
        assert og.shape == (E, N, 12 + B * A)
        assert_rows_close(og, fx[f"{case}_obs"][:, t], rtol + F32_ULP, f"{case} t={t} ")
        fg, ig = get_state(env)
        want = ref_state[:, t].reshape(E * N, 16)
        for g, cols in (("pos", slice(0, 3)), ("quat", slice(3, 7)), ("vel", slice(7, 10)), ("omega", slice(10, 13)),
                        ("angv", slice(13, 16))):
            rows = [idx[n] for n in GROUPS[g]]
            d = np.linalg.norm(fg[rows].T - want[:, cols], axis=1)
            err = d / np.maximum(np.linalg.norm(want[:, cols], axis=1), FLOORS[g])
            assert err.max() <= rtol, f"{case} t={t} {g}: max rel err {err.max():.3e}"
        assert (ig[iidx["step_counter"]] == 8 * (t + 1)).all() and (ig[iidx["ring_head"]] == 1).all()
        np.testing.assert_allclose(rew.cpu().numpy(), fx[f"{case}_rew"][:, t], rtol=rtol + F32_ULP, atol=1e-5 * rtol / 1e-4)
        np.testing.assert_array_equal(te.cpu().numpy(), fx[f"{case}_term"][:, t])
        trunc_mismatches_at_threshold(tr.cpu().numpy(), fx[f"{case}_trunc"][:, t], fx[f"{case}_obs"][:, t],
                                      rtol + F32_ULP)
    env.close()


# ---------------------------------------------------------------------------------------------
# C2  uncoupled modes: every drone against the unchanged single-drone oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("E,N", [(37, 3), (9, 8), (70, 2), (1, 5)])
@pytest.mark.parametrize("physics", UNCOUPLED)
def test_uncoupled_against_single_drone_oracle(physics, E, N, precision):
    rtol = RTOL[precision]
    rng = np.random.default_rng(1000 * UNCOUPLED.index(physics) + 10 * E + N)
    env = MultiHoverAviary(num_drones=N, physics=physics, num_envs=E, precision=precision, autoreset=False)
    G = {2: 2, 3: 4, 5: 8, 8: 8}[N]
    assert env.kernel_name == f"multihover_step<{'f64' if precision == 'fp64' else 'f32'},{physics.name},A4,G{G}>"
    orcs = [hover_oracle(env, n) for n in range(N)]
    idx, iidx, names = field_index(env)
    assert orcs[0].field_names()[0] == names
    f, i = random_multi_state(rng, env)
    put_state(env, f, i)
    for n, o in enumerate(orcs):
        o.set_state(f[:, n::N].copy(), i[:, n::N].copy())
    active = active_fields(physics)
    real = real_of(env)
    for t in range(3):
        act = rng.uniform(-1, 1, (E, N, 4)).astype(np.float32)
        outs = [o.step(act[:, n:n + 1]) for n, o in enumerate(orcs)]
        obs, rew, te, tr, _ = env.step(torch.from_numpy(act))
        torch.cuda.synchronize()
        og = obs.cpu().numpy()
        fg, ig = get_state(env)
        fo = np.zeros_like(fg); io = np.zeros_like(ig)
        for n, o in enumerate(orcs):
            fo[:, n::N], io[:, n::N] = o.get_state()
        assert_state_close(fg, fo, idx, names, rtol, active, f"t={t} ")
        np.testing.assert_array_equal(ig, io)
        oo = np.concatenate([out[0] for out in outs], axis=1)            # [E, N, D]
        assert_rows_close(og, oo, rtol + F32_ULP, f"t={t} ")
        rew_o = np.zeros(E)
        for out in outs:
            rew_o = rew_o + out[1].astype(np.float64)
        np.testing.assert_allclose(rew.cpu().numpy(), rew_o, rtol=rtol + N * F32_ULP, atol=1e-5 * rtol / 1e-4)
        te_o, tr_o = flags_numpy(oo, env.TARGET_POS, io[iidx["step_counter"]][::N] - env.PYB_STEPS_PER_CTRL)
        np.testing.assert_array_equal(te.cpu().numpy(), te_o)
        trunc_mismatches_at_threshold(tr.cpu().numpy(), tr_o, oo, rtol + F32_ULP)
        # teacher forcing: the oracles' state into both
        fo = fo.astype(real).astype(np.float64)
        put_state(env, fo, io)
        for n, o in enumerate(orcs):
            o.set_state(fo[:, n::N].copy(), io[:, n::N].copy())
    env.close()


# ---------------------------------------------------------------------------------------------
# C3  one drone per env is HoverAviary, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("physics", UNCOUPLED)
def test_one_drone_is_hover_aviary(physics, precision):
    E = 67
    rng = np.random.default_rng(300 + UNCOUPLED.index(physics))
    kw = dict(physics=physics, num_envs=E, precision=precision, autoreset=False)
    multi = MultiHoverAviary(num_drones=1, initial_xyzs=[[0, 0, 0]], **kw)
    hover = HoverAviary(initial_xyzs=[0, 0, 0], **kw)
    np.testing.assert_array_equal(multi.TARGET_POS, [[0, 0, 1]])
    assert multi.state_field_names() == hover.state_field_names()
    f, i = random_multi_state(rng, multi, spread=0.2, tilt=0.1, vel=0.2, omega=0.5)
    put_state(multi, f, i)
    put_state(hover, f, i)
    for t in range(20):
        act = torch.from_numpy(rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)).to(multi.device)
        om, rm, _, _, _ = multi.step(act)
        oh, rh, _, _, _ = hover.step(act)
        fm, im = multi.get_state()
        fh, ih = hover.get_state()
        assert torch.equal(fm, fh), f"t={t}: state differs in {int((fm != fh).sum())} values"
        assert torch.equal(im, ih)
        assert torch.equal(om, oh) and torch.equal(rm, rh)
    multi.close(); hover.close()


# ---------------------------------------------------------------------------------------------
# C4 / C5  downwash
# ---------------------------------------------------------------------------------------------
def stacked_state(rng, env, equal_z=True, vel=0.5, beta_margin=0.02):
    """drones of an env stacked above each other: lateral offsets in [0, 0.15] m, vertical gaps in
    [0.15, 0.5] m (or exactly 0: equal z, no force either way), lowest at z >= 0.5, in a random order of
    the drone index; no pair's |dz| in (0, 0.1) (ill-conditioned) or within beta_margin of 0.6875 (beta = 0);
    link_quat = quat"""
    E, N = env.num_envs, env.NUM_DRONES
    idx, iidx, names = field_index(env)
    f = np.zeros((len(names), E * N))
    i = np.zeros((3, E * N), np.int32)
    pos = np.zeros((E, N, 3))
    for e in range(E):
        while True:
            gaps = rng.uniform(0.15, 0.5, N - 1)
            if equal_z:
                gaps[rng.random(N - 1) < 0.25] = 0.0
            z = 0.5 + rng.uniform(0, 0.2) + np.concatenate([[0.0], np.cumsum(gaps)])
            dz = np.abs(z[:, None] - z[None, :])
            if not (((dz > 0) & (dz < 0.1)).any() or (np.abs(dz - 0.6875) < beta_margin).any()):
                break
        z = z[rng.permutation(N)]
        pos[e] = np.stack([rng.uniform(0, 0.15, N), rng.uniform(0, 0.15, N), z], 1)
    pos = pos.reshape(E * N, 3)
    rpy = rng.uniform(-0.2, 0.2, (E * N, 3)) * np.array([1, 1, 4])
    q = np.array([O.quat_from_euler(r) for r in rpy])
    v = rng.uniform(-vel, vel, (E * N, 3))
    w = rng.uniform(-1, 1, (E * N, 3))
    for k, ax in enumerate("xyz"):
        f[idx[f"pos_{ax}"]] = pos[:, k]; f[idx[f"vel_{ax}"]] = v[:, k]; f[idx[f"omega_{ax}"]] = w[:, k]
    for k, ax in enumerate("xyzw"):
        f[idx[f"quat_{ax}"]] = q[:, k]; f[idx[f"link_quat_{ax}"]] = q[:, k]
    for k in range(4):
        f[idx[f"last_rpm_{k}"]] = rng.uniform(0.8, 1.2, E * N) * 16364.0
    f = f.astype(real_of(env)).astype(np.float64)
    return f, i


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("N", [3, 5, 8])
@pytest.mark.parametrize("physics", DOWNWASH)
def test_downwash_one_substep(physics, N, precision):
    """S = 1: the state after the step is the single-drone oracle's (no neighbour, no downwash) plus
    dv = dt F / m, dp = dt dv, F the oracle's own force assembly of the N drones minus the drone's alone.
    N = 5 is the smallest with the G = 8 ds_bpermute exchange, three inactive lanes per group and masked
    partners that wrap around the group ((n + r) & 7)."""
    E, rtol = 32, RTOL[precision]
    rng = np.random.default_rng(400 + N + DOWNWASH.index(physics))
    env = MultiHoverAviary(num_drones=N, physics=physics, pyb_freq=240, ctrl_freq=240, num_envs=E,
                           precision=precision, autoreset=False)
    assert env.PYB_STEPS_PER_CTRL == 1
    idx, iidx, names = field_index(env)
    f, i = stacked_state(rng, env)
    put_state(env, f, i)
    act = rng.uniform(-1, 1, (E, N, 4)).astype(np.float32)
    orcs = [hover_oracle(env, n) for n in range(N)]
    fo = np.zeros_like(f)
    for n, o in enumerate(orcs):
        o.set_state(f[:, n::N].copy(), i[:, n::N].copy())
        o.step(act[:, n:n + 1])
        fo[:, n::N] = o.get_state()[0]
    cfg = orcs[0].cfg
    rows13 = [idx[k] for k in ("pos_x", "pos_y", "pos_z", "quat_x", "quat_y", "quat_z", "quat_w", "vel_x", "vel_y",
                               "vel_z", "omega_x", "omega_y", "omega_z")]
    prev_rows = [idx[f"last_rpm_{k}"] for k in range(4)]
    dt, m = 1.0 / 240, cfg.drone.m
    pushed = 0
    for e in range(E):
        states = f[rows13][:, e * N:(e + 1) * N].T.copy()                 # [N, 13]
        for n in range(N):
            rpm = O.hover_rpm(cfg, act[e, n])
            prev = f[prev_rows, e * N + n]
            lf_all, lt_all = O.force_assembly(cfg, states, n, rpm, prev)
            lf_one, lt_one = O.force_assembly(cfg, states[n:n + 1], 0, rpm, prev)
            np.testing.assert_array_equal(lt_all[4], lt_one[4])           # the downwash adds no torque
            np.testing.assert_array_equal(lf_all[:4], lf_one[:4])
            x, y, z, w = states[n, 3:7]                                   # link basis = the pose's (link_quat := quat)
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
            F = R @ (lf_all[4] - lf_one[4])
            pushed += np.linalg.norm(F) > 0.01 * m * cfg.gravity
            dv = dt * F / m
            c = e * N + n
            for k, ax in enumerate("xyz"):
                fo[idx[f"vel_{ax}"], c] += dv[k]
                fo[idx[f"pos_{ax}"], c] += dt * dv[k]
    assert pushed >= E * N // 2, f"only {pushed} of {E * N} drones feel a downwash above 1 % of their weight"
    env.step(torch.from_numpy(act))
    torch.cuda.synchronize()
    fg, ig = get_state(env)
    assert_state_close(fg, fo, idx, names, rtol, active_fields(physics), f"{physics.name} N={N} ")
    env.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("N", [3, 8])
@pytest.mark.parametrize("physics", DOWNWASH)
def test_downwash_exchange_every_substep(physics, N, precision):
    """one env.step of 8 sub-steps (240 / 30 Hz) against eight env.steps of one sub-step (240 / 240 Hz)
    with the same constant action: a kernel that read the neighbours once per launch misses by ~1e-3"""
    E, rtol = 32, RTOL[precision]
    rng = np.random.default_rng(500 + N + DOWNWASH.index(physics))
    kw = dict(num_drones=N, physics=physics, pyb_freq=240, num_envs=E, precision=precision, autoreset=False)
    coarse = MultiHoverAviary(ctrl_freq=30, **kw)
    fine = MultiHoverAviary(ctrl_freq=240, **kw)
    idx_c, _, names_c = field_index(coarse)
    idx_f, _, names_f = field_index(fine)
    # (the drones move up to 2 * 0.5 / 30 m against each other during the step: distinct heights, and the
    # margins of stacked_state widened by that)
    fc, ic = stacked_state(rng, coarse, equal_z=False, vel=0.5, beta_margin=0.06)
    ff = np.zeros((len(names_f), E * N))
    body = [n for n in names_c if not n.startswith("ring_")]
    for nme in body:
        ff[idx_f[nme]] = fc[idx_c[nme]]
    put_state(coarse, fc, ic)
    put_state(fine, ff, ic)
    act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 4)).astype(np.float32))
    coarse.step(act)
    for _ in range(8):
        fine.step(act)
    torch.cuda.synchronize()
    gc, _ = get_state(coarse)
    gf, _ = get_state(fine)
    for g in sorted(active_fields(physics)):
        a = gc[[idx_c[n] for n in GROUPS[g]]]
        b = gf[[idx_f[n] for n in GROUPS[g]]]
        err = np.linalg.norm(a - b, axis=0) / np.maximum(np.linalg.norm(b, axis=0), FLOORS[g])
        assert err.max() <= rtol, f"{g}: max rel err {err.max():.3e}"
    coarse.close(); fine.close()


# ---------------------------------------------------------------------------------------------
# C6  terminated is a sum over the drones; the bounds are 2.0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_termination_is_a_sum_and_bounds_are_two(precision):
    E, N = 4, 2
    env = MultiHoverAviary(num_drones=N, physics=Physics.PYB, num_envs=E, precision=precision, autoreset=False)
    idx, iidx, names = field_index(env)
    f = np.zeros((len(names), E * N))
    pos = np.tile(env.TARGET_POS, (E, 1))
    pos[2:4, 0] += 6e-5            # env 1: both drones 6e-5 m off (each < 1e-4, the sum 1.2e-4)
    pos[4, 0] = 1.7                # env 2: inside MultiHoverAviary's 2.0 (outside HoverAviary's 1.5)
    pos[6, 0] = 2.1                # env 3: outside
    for k, ax in enumerate("xyz"):
        f[idx[f"pos_{ax}"]] = pos[:, k]
    f[idx["quat_w"]] = 1.0
    f[idx["link_quat_w"]] = 1.0
    put_state(env, f, np.zeros((3, E * N), np.int32))
    _, _, te, tr, _ = env.step(torch.zeros((E, N, 4)))
    assert te.cpu().tolist() == [True, False, False, False]
    assert tr.cpu().tolist() == [False, False, False, True]
    env.close()


# ---------------------------------------------------------------------------------------------
# C7  auto-reset per env, Philox per (env, drone, episode), shard and batch invariance
# ---------------------------------------------------------------------------------------------
def test_autoreset_whole_env():
    E, N = 6, 3
    rng = np.random.default_rng(70)
    kw = dict(num_drones=N, physics=Physics.PYB, num_envs=E, precision="fp64")
    env = MultiHoverAviary(autoreset=True, **kw)
    ref = MultiHoverAviary(autoreset=False, **kw)
    idx, iidx, names = field_index(env)
    f, i = random_multi_state(rng, env, spread=0.1, tilt=0.05)
    f[idx["pos_x"], 1 * N + 2] = 2.5          # env 1 leaves through its last drone
    f[idx["pos_x"], 4 * N + 0] = -2.5         # env 4 through its first
    put_state(env, f, i)
    put_state(ref, f, i)
    act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 4)).astype(np.float32))
    obs, rew, te, tr, info = env.step(act)
    obs_r, rew_r, te_r, tr_r, _ = ref.step(act)
    done = [False, True, False, False, True, False]
    assert tr.cpu().tolist() == done and tr_r.cpu().tolist() == done and not te.any()
    assert torch.equal(rew, rew_r)
    og, orr, tobs = obs.cpu().numpy(), obs_r.cpu().numpy(), info["terminal_observation"].cpu().numpy()
    fg, ig = get_state(env)
    fr, ir = get_state(ref)
    B, A = env.ACTION_BUFFER_SIZE, 4
    for e in range(E):
        cols = slice(e * N, (e + 1) * N)
        if not done[e]:
            np.testing.assert_array_equal(og[e], orr[e])
            np.testing.assert_array_equal(fg[:, cols], fr[:, cols])
            np.testing.assert_array_equal(ig[:, cols], ir[:, cols])
            continue
        np.testing.assert_array_equal(tobs[e], orr[e])                     # terminal rows: the pre-reset obs, all N
        want = np.zeros((N, 12 + B * A), np.float32)
        want[:, :3] = env.INIT_XYZS
        np.testing.assert_array_equal(og[e], want)                          # every drone back at its start, ring cleared
        for k, ax in enumerate("xyz"):
            np.testing.assert_array_equal(fg[idx[f"pos_{ax}"], cols], env.INIT_XYZS[:, k])
            np.testing.assert_array_equal(fg[idx[f"vel_{ax}"], cols], 0)
        ring = [k for k, n in enumerate(names) if n.startswith("ring_")]
        assert not fg[ring][:, cols].any()
        assert (ig[iidx["step_counter"], cols] == 0).all()
        assert (ig[iidx["episode"], cols] == i[iidx["episode"], e * N] + 1).all()
    env.close(); ref.close()


def test_reset_noise_per_drone():
    E, N = 16, 3
    env = MultiHoverAviary(num_drones=N, num_envs=E, precision="fp64", seed=5,
                           init_noise={"xyz": 0.05, "rpy": 0.1, "vel": 0.2, "omega": 0.3})
    obs, _ = env.reset()
    o = obs.cpu().numpy().astype(np.float64)
    d = o[:, :, :3] - env.INIT_XYZS[None]
    assert np.abs(d).max() <= 0.05 + 1e-6 and np.abs(o[:, :, 3:6]).max() <= 0.1 + 1e-6
    assert np.abs(o[:, :, 6:9]).max() <= 0.2 + 1e-6
    assert not o[:, :, 12:].any()
    for a in range(N):                       # distinct draws across the drones of an env, and across envs
        for b in range(a + 1, N):
            assert (np.abs(d[:, a] - d[:, b]).max(axis=1) > 1e-4).all()
    assert (np.abs(d[0] - d[1]).max(axis=1) > 1e-4).all()
    env.close()


NOISE = {"xyz": 0.02, "rpy": 0.3, "vel": 0.2, "omega": 0.5}


def stack_xyzs(N):
    """initial positions 0.18 m above each other (the downwash acts, well away from its dz -> 0 pole)"""
    return [[0.05 * n, 0.0, 0.3 + 0.18 * n] for n in range(N)]


def run_steps(env, acts):
    out = []
    env.reset()
    for a in acts:
        obs, rew, te, tr, info = env.step(a)
        out.append((obs.clone(), rew.clone(), te.clone(), tr.clone(), info["terminal_observation"].clone()))
    env.close()
    return out


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_shards_are_bit_identical(precision):
    N, T = 3, 40
    rng = np.random.default_rng(71)
    kw = dict(num_drones=N, initial_xyzs=stack_xyzs(N), physics=Physics.PYB_DW, precision=precision, seed=9,
              init_noise=NOISE)
    acts = [torch.from_numpy(rng.uniform(-1, 1, (8, N, 4)).astype(np.float32)).cuda() for _ in range(T)]
    whole = run_steps(MultiHoverAviary(num_envs=8, **kw), acts)
    lo = run_steps(MultiHoverAviary(num_envs=4, env_offset=0, **kw), [a[:4].contiguous() for a in acts])
    hi = run_steps(MultiHoverAviary(num_envs=4, env_offset=4, **kw), [a[4:].contiguous() for a in acts])
    resets = 0
    for t in range(T):
        for k in range(5):
            assert torch.equal(whole[t][k], torch.cat([lo[t][k], hi[t][k]])), f"t={t} output {k}"
        resets += int((whole[t][2] | whole[t][3]).sum())
    assert resets >= 4, "the run is meant to cross auto-resets"


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("N", [3, 8])
def test_batch_invariance(N, precision):
    T = 20
    rng = np.random.default_rng(72)
    kw = dict(num_drones=N, initial_xyzs=stack_xyzs(N), physics=Physics.PYB_GND_DRAG_DW, precision=precision, seed=11,
              init_noise=NOISE)
    acts = [torch.from_numpy(rng.uniform(-1, 1, (133, N, 4)).astype(np.float32)).cuda() for _ in range(T)]
    big = run_steps(MultiHoverAviary(num_envs=133, **kw), acts)
    small = run_steps(MultiHoverAviary(num_envs=5, **kw), [a[:5].contiguous() for a in acts])
    for t in range(T):
        for k in range(5):
            assert torch.equal(big[t][k][:5], small[t][k]), f"t={t} output {k}"


# ---------------------------------------------------------------------------------------------
# C8  SB3 VecEnv, helpers
# ---------------------------------------------------------------------------------------------
def test_vec_env():
    from gym_pybullet_adrp_amd.vec_env import MultiHoverAviaryVec
    E, N = 6, 2
    kw = dict(num_drones=N, seed=3, init_noise=NOISE)
    vec = MultiHoverAviaryVec(n_envs=E, **kw)
    env = MultiHoverAviary(num_envs=E, **kw)
    D = 72
    assert vec.observation_space.shape == (N, D) and vec.action_space.shape == (N, 4) and vec.num_envs == E
    o = vec.reset()
    oe, _ = env.reset()
    assert o.shape == (E, N, D) and o.dtype == np.float32
    np.testing.assert_array_equal(o, oe.cpu().numpy())
    rng = np.random.default_rng(8)
    seen = 0
    for t in range(60):
        act = rng.uniform(-1, 1, (E, N, 4)).astype(np.float32)
        o, r, d, infos = vec.step(act)
        oe, re, te, tr, info = env.step(act)
        assert o.shape == (E, N, D) and r.shape == (E,) and d.shape == (E,) and len(infos) == E
        np.testing.assert_array_equal(o, oe.cpu().numpy())
        np.testing.assert_array_equal(r, re.cpu().numpy())
        np.testing.assert_array_equal(d, (te | tr).cpu().numpy())
        for e in np.flatnonzero(d):
            tob = infos[e]["terminal_observation"]
            assert tob.shape == (N, D)
            np.testing.assert_array_equal(tob, info["terminal_observation"][e].cpu().numpy())
            assert infos[e]["TimeLimit.truncated"] == bool(tr[e] and not te[e])
            seen += 1
        for e in np.flatnonzero(~d):
            assert "terminal_observation" not in infos[e]
    assert seen >= 1, "no episode ended in 60 steps"
    vec.close(); env.close()


def test_adjacency_and_min_pair_distance():
    E, N = 3, 3
    env = MultiHoverAviary(num_drones=N, num_envs=E, neighbourhood_radius=0.3, autoreset=False)
    env.reset()
    p = env.INIT_XYZS
    dist = np.linalg.norm(p[:, None] - p[None], axis=-1)
    adj = env.adjacency_matrix()
    assert adj.shape == (E, N, N)
    np.testing.assert_array_equal(adj[0].cpu().numpy(), ((dist < 0.3) | np.eye(N, dtype=bool)).astype(float))
    mpd = env.min_pair_distance()
    assert mpd.shape == (E,)
    np.testing.assert_allclose(mpd.cpu().numpy(), 4 * env.L * np.sqrt(2), rtol=1e-12)
    env.close()
