"""The hover step with field addressing by 32-bit offsets, flat props compiled out and the roll on the
reset-helper wave ("Off the chain wave"): each item changes who computes a value or how an
address is formed, none changes a value.  Needs an MI355X: -m gpu.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs.hover import HoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils import abi  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Physics  # noqa: E402
from oracle import oracle as O  # noqa: E402

from test_hover_gpu import active_fields, compare_state, pair, random_states  # noqa: E402

BENCH_NOISE = {"xyz": 0.1, "rpy": 0.05, "vel": 0.1, "omega": 0.1}   # bench.py's init_noise


def free_run(E, steps, acts, **kw):
    """`steps` auto-reset env.steps of a fresh env: per step (obs, terminal obs, reward, terminated,
    truncated) as numpy copies, and the final state"""
    env = HoverAviary(num_envs=E, initial_xyzs=[0, 0, 1.0], init_noise=BENCH_NOISE, **kw)
    name = env.kernel_name
    env.reset()
    seq = []
    for t in range(steps):
        obs, rew, te, tr, info = env.step(acts[t].to(env.device))
        seq.append((obs.reshape(E, -1).cpu().numpy().copy(), info["terminal_observation"].reshape(E, -1).cpu().numpy().copy(),
                    rew.reshape(E).cpu().numpy().copy(), te.reshape(E).cpu().numpy().copy(), tr.reshape(E).cpu().numpy().copy()))
    f, i = env.get_state()
    f, i = f.cpu().numpy().copy(), i.cpu().numpy().copy()
    env.close()
    return name, seq, (f, i)


@pytest.mark.parametrize("physics", [Physics.PYB, Physics.PYB_GND_DRAG_DW])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_flat_props_against_generic(monkeypatch, precision, physics):
    """The compiled-in drone's props lie in the body plane, and the `cf2x` kernels drop the P.z sum and
    the two P.z products of the torque.  fma(0, x, c) and c - 0 y equal c but for the sign of an exact
    zero, so the default handle must give the bits of the generic kernel (ADRP_HOVER_GENERIC=1: the same
    constants from device memory, the full expression): obs, reward, both flags, the terminal rows of
    done envs and the final state, over 40 auto-reset steps of seeded U[-1, 1] actions at E = 128.
    (The parent commit's two kernels, which both keep the products, also agree in every element here.)"""
    E, T = 128, 40
    acts = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (T, E, 1, 4)).astype(np.float32))
    monkeypatch.delenv("ADRP_HOVER_GENERIC", raising=False)
    name_c, seq_c, st_c = free_run(E, T, acts, physics=physics, precision=precision, seed=11)
    monkeypatch.setenv("ADRP_HOVER_GENERIC", "1")
    name_g, seq_g, st_g = free_run(E, T, acts, physics=physics, precision=precision, seed=11)
    assert name_c.endswith(",cf2x>") and name_g.endswith(",generic>"), (name_c, name_g)
    dones = 0
    for t, ((o1, t1, r1, te1, tr1), (o0, t0, r0, te0, tr0)) in enumerate(zip(seq_c, seq_g)):
        np.testing.assert_array_equal(te1, te0, err_msg=f"step {t}")
        np.testing.assert_array_equal(tr1, tr0, err_msg=f"step {t}")
        np.testing.assert_array_equal(o1, o0, err_msg=f"step {t}")
        np.testing.assert_array_equal(r1, r0, err_msg=f"step {t}")
        d = te1 | tr1
        dones += int(d.sum())
        np.testing.assert_array_equal(t1[d], t0[d], err_msg=f"step {t}")
    assert dones > 0
    np.testing.assert_array_equal(st_c[0], st_g[0])
    np.testing.assert_array_equal(st_c[1], st_g[1])


def raised_props(cfg, dz=0.005):
    """props 0 and 2 lifted by dz out of the body plane"""
    cfg.drone.prop_pos[0][2] = dz
    cfg.drone.prop_pos[2][2] = dz
    return cfg


def unequal_rpm_actions(rng, E):
    """the four motors far apart, so that P = sum f_i p_i has a z part of the size of its x and y parts"""
    base = np.array([0.9, -0.7, 0.3, -0.2])
    return (base + rng.uniform(-0.1, 0.1, (E, 1, 4))).astype(np.float32)


def test_raised_props_oracle_sensitivity():
    """CPU only (two oracle runs): lifting props 0 and 2 by 5 mm moves the oracle's own angular velocity
    after 8 steps by far more than the 1e-9 bar that test_raised_props_still_count holds the kernel to,
    so a kernel that dropped P.z for this drone could not pass it"""
    E = 64
    rng = np.random.default_rng(21)
    cfg = _lib.default_config(abi.TASK_HOVER)
    cfg.num_envs, cfg.precision, cfg.autoreset, cfg.action_buffer_size = E, 1, 0, 15
    flat, lifted = O.Oracle(cfg.copy()), O.Oracle(raised_props(cfg.copy()))
    flat.reset()
    lifted.reset()
    lifted.set_state(*flat.get_state())
    for _ in range(8):
        act = unequal_rpm_actions(rng, E)
        flat.step(act)
        lifted.step(act)
    names, _ = flat.field_names()
    rows = [names.index(f"omega_{a}") for a in "xyz"]
    ff, fl = flat.get_state()[0], lifted.get_state()[0]
    rel = np.linalg.norm(ff[rows] - fl[rows], axis=0) / np.maximum(np.linalg.norm(fl[rows], axis=0), 1e-3)
    print(f"oracle, flat against lifted props: omega differs by {rel.min():.2e} .. {rel.max():.2e} relative")
    assert rel.min() > 1e-5   # four orders above the 1e-9 bar, in every env


def test_raised_props_still_count():
    """A drone whose props 0 and 2 sit 5 mm above the body plane selects the generic kernel, which keeps
    the whole P x m3: teacher-forced against the float64 oracle at the fp64 bar of test_hover_gpu.py
    (1e-9 of max(|x|, floor) per state vector), E = 64, 8 steps, unequal RPMs"""
    E = 64
    rng = np.random.default_rng(22)
    env, _ = pair(E, Physics.PYB, precision="fp64", autoreset=False)
    env.h.close()
    env.cfg = raised_props(env.cfg)
    env.h = _lib.Handle(env.cfg, env.device.index)
    env.h.bind(env._obs, env._rew, env._term, env._trunc, env._tobs)
    assert "cf2x" not in env.kernel_name, env.kernel_name
    orc = O.Oracle(env.cfg.copy())
    env.reset()
    orc.reset()
    random_states(rng, E, env, orc)
    real = np.float64
    for _ in range(8):
        act = unequal_rpm_actions(rng, E)
        orc.step(act)
        env.step(torch.from_numpy(act))
        torch.cuda.synchronize()
        worst = compare_state(env, orc, 1e-9, active_fields(Physics.PYB))
        f, i = orc.get_state()
        env.set_state(torch.from_numpy(f.astype(real)), torch.from_numpy(i))
    print("worst relative errors (last step):", {g: f"{v:.2e}" for g, v in sorted(worst.items())})
    env.close()


@pytest.fixture(scope="module")
def addressing_reference():
    """256 random fp64 states and one auto-reset step of them inside an E = 256 handle, computed once:
    state, ints and every output after the step"""
    E = 256
    rng = np.random.default_rng(33)
    env, orc = pair(E, Physics.PYB, precision="fp64", autoreset=True, seed=5, initial_xyzs=[0, 0, 1.0], init_noise=BENCH_NOISE)
    env.reset()
    f, i = random_states(rng, E, env, orc, tilt=0.3)
    names, inames = env.state_field_names()
    i[inames.index("ring_head")] = 7          # (one head for all: what every real run has)
    i[inames.index("step_counter")][::5] = 1928   # a fifth of the envs run out of time in this step
    act = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    out = step_once(env, f, i, act)
    env.close()
    return f, i, act, out


def step_once(env, f, i, act):
    E = env.num_envs
    env.set_state(torch.from_numpy(f), torch.from_numpy(i))
    obs, rew, te, tr, info = env.step(torch.from_numpy(act))
    torch.cuda.synchronize()
    fs, is_ = env.get_state()
    return {"obs": obs.reshape(E, -1).cpu().numpy().copy(), "tobs": info["terminal_observation"].reshape(E, -1).cpu().numpy().copy(),
            "rew": rew.cpu().numpy().copy(), "term": te.cpu().numpy().copy(), "trunc": tr.cpu().numpy().copy(),
            "f": fs.cpu().numpy().copy(), "i": is_.cpu().numpy().copy()}


@pytest.mark.parametrize("E", [64, 65, 128, 193])
def test_addressing_batch_sizes(addressing_reference, E):
    """The field offsets depend on E (the stride) and on the env (the lane's first offset): the first E of
    the reference's envs, stepped in a handle of E envs, give the reference's bits in the state, the ints
    and every output.  E = 64 and 128: full blocks of the staged kernel with its helper waves; 65 and
    193 = 192 + 1: the row-store kernel with a ragged last wave (test_fp64_batch_invariance's pattern).
    The reset of a done env draws from the env's own Philox stream (env index, episode), so it is the same
    in both handles."""
    f, i, act, ref = addressing_reference
    env = HoverAviary(physics=Physics.PYB, precision="fp64", num_envs=E, seed=5, initial_xyzs=[0, 0, 1.0], init_noise=BENCH_NOISE)
    env.reset()
    got = step_once(env, np.ascontiguousarray(f[:, :E]), np.ascontiguousarray(i[:, :E]), act[:E])
    env.close()
    done = ref["term"][:E] | ref["trunc"][:E]
    assert done.any() and not done.all()
    for k in ("term", "trunc", "rew", "obs", "tobs"):   # (terminal rows: written for done envs, zeros otherwise, in both)
        np.testing.assert_array_equal(got[k], ref[k][:E], err_msg=k)
    assert got["tobs"][done].any() and not got["tobs"][~done].any()
    np.testing.assert_array_equal(got["f"], ref["f"][:, :E])
    np.testing.assert_array_equal(got["i"], ref["i"][:, :E])


def oracle_done_blocks(E, T, acts, seed):
    """the CPU oracle's done flags of the run of test_done_lanes, per step and 64-env block"""
    cfg = _lib.default_config(abi.TASK_HOVER)
    cfg.num_envs, cfg.precision, cfg.autoreset, cfg.action_buffer_size, cfg.seed = E, 1, 1, 15, seed
    abi.set_vec(cfg.init_xyz[0], np.array([0, 0, 1.0]))
    for dst, key in ((cfg.init_xyz_noise, "xyz"), (cfg.init_rpy_noise, "rpy"), (cfg.init_vel_noise, "vel"),
                     (cfg.init_omega_noise, "omega")):
        abi.set_vec(dst, np.full(3, BENCH_NOISE[key]))
    orc = O.Oracle(cfg)
    orc.reset()
    per = []
    for t in range(T):
        _, _, te, tr, _ = orc.step(acts[t])
        per.append((te | tr).reshape(E // 64, 64).any(1))
    return np.array(per)


def test_done_lanes(monkeypatch):
    """Who writes which part of a row changes with the helper waves: 40 auto-reset steps at E = 128 (two
    blocks) with the helpers, without them (ADRP_RESET_HELPER=0) and on the row-store kernel
    (ADRP_STAGE_ROWS=0) give the same bits in obs, reward, both flags and the terminal rows of done envs
    (test_reset_helper_same_results' pattern at a shape that runs in seconds), and an env that was never
    done still has the terminal row that the env's construction left (zeros).  Seed 99: on the CPU
    oracle the run has steps where both blocks hold a done env and steps where one holds none."""
    E, T, seed = 128, 40, 99
    acts_np = np.random.default_rng(seed).uniform(-1, 1, (T, E, 1, 4)).astype(np.float32)
    per = oracle_done_blocks(E, T, acts_np, seed)
    assert per.all(1).any() and (~per).any(1).any(), per.sum(1).tolist()
    acts = torch.from_numpy(acts_np)
    runs = []
    for helper, stage in (("1", "1"), ("0", "1"), ("1", "0")):
        monkeypatch.setenv("ADRP_RESET_HELPER", helper)
        monkeypatch.setenv("ADRP_STAGE_ROWS", stage)
        runs.append(free_run(E, T, acts, physics=Physics.PYB, precision="fp64", seed=seed))
    _, base, base_state = runs[0]
    ever = np.zeros(E, bool)
    both_kinds = [False, False]
    for t, (o1, t1, r1, te1, tr1) in enumerate(base):
        d1 = te1 | tr1
        blocks = d1.reshape(E // 64, 64).any(1)
        both_kinds[0] |= bool(blocks.all())
        both_kinds[1] |= bool((~blocks).any())
        ever |= d1
        assert not t1[~ever].any(), f"step {t}: a terminal row of an env that was never done was written"
        for _, other, _ in runs[1:]:
            o0, t0, r0, te0, tr0 = other[t]
            np.testing.assert_array_equal(te1, te0, err_msg=f"step {t}")
            np.testing.assert_array_equal(tr1, tr0, err_msg=f"step {t}")
            np.testing.assert_array_equal(o1, o0, err_msg=f"step {t}")
            np.testing.assert_array_equal(r1, r0, err_msg=f"step {t}")
            np.testing.assert_array_equal(t1[ever], t0[ever], err_msg=f"step {t}")
            assert not t0[~ever].any()
    assert all(both_kinds), both_kinds
    for _, _, st in runs[1:]:
        np.testing.assert_array_equal(st[0], base_state[0])
        np.testing.assert_array_equal(st[1], base_state[1])
