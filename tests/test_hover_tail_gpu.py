"""The tail of the hover step ("The tail"): in the fp64 kernels with angle helper waves the
terminal rows of done envs leave in two parts (the chain wave's done lanes store the kinematic columns, the
helper waves copy the ring columns of the listed rows out of the staged block), and the helper waves
evaluate lean forms of atan2 / asin with a whole-wave fall-back to the full functions.  Neither changes a
value: every case here is held, bit for bit, to the row-store kernel without helper waves
(ADRP_STAGE_ROWS=0, ADRP_RESET_HELPER=0), whose angle and done paths are the ones from before.  The staged
kernels without angle helpers (fp32, ADRP_RESET_HELPER=0) go through the same cases.
Needs an MI355X: -m gpu.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.envs.hover import HoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Physics  # noqa: E402
from oracle import oracle as O  # noqa: E402

from test_hover_gpu import pair, random_states  # noqa: E402

BENCH_NOISE = {"xyz": 0.1, "rpy": 0.05, "vel": 0.1, "omega": 0.1}   # bench.py's init_noise
SWITCHES = ("ADRP_STAGE_ROWS", "ADRP_RESET_HELPER")
REFERENCE = {"ADRP_STAGE_ROWS": "0", "ADRP_RESET_HELPER": "0"}
# the kernels under test: staged rows with the helper waves (the benched one), staged rows alone
STAGED = {"helpers": {}, "staged": {"ADRP_RESET_HELPER": "0"}}
SENTINEL = 12345.0    # what a terminal row holds before any step wrote it
KEYS = ("term", "trunc", "rew", "obs", "tobs", "f", "i")


def make_env(monkeypatch, E, precision, switches, **kw):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    kw.setdefault("seed", 5)
    env = HoverAviary(physics=Physics.PYB, precision=precision, num_envs=E, initial_xyzs=[0, 0, 1.0],
                      init_noise=BENCH_NOISE, **kw)
    env.reset()
    return env


def outputs(env, ret):
    E = env.num_envs
    obs, rew, te, tr, info = ret
    torch.cuda.synchronize()
    fs, is_ = env.get_state()
    return {"obs": obs.reshape(E, -1).cpu().numpy().copy(), "tobs": info["terminal_observation"].reshape(E, -1).cpu().numpy().copy(),
            "rew": rew.reshape(E).cpu().numpy().copy(), "term": te.reshape(E).cpu().numpy().copy(),
            "trunc": tr.reshape(E).cpu().numpy().copy(), "f": fs.cpu().numpy().copy(), "i": is_.cpu().numpy().copy()}


def step_once(env, f, i, act):
    """one env.step from the state (f, i), every terminal row holding the sentinel before it"""
    env.set_state(torch.from_numpy(f), torch.from_numpy(i))
    env._tobs.fill_(SENTINEL)
    return outputs(env, env.step(torch.from_numpy(act)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, ref, what, rows=None):
    """bit for bit; a NaN must be a NaN in both (its payload is not held)"""
    for k in KEYS:
        g, r = got[k], ref[k]
        if rows is not None:
            g, r = (g[:, rows], r[:, rows]) if k in ("f", "i") else (g[rows], r[rows])
        if g.dtype.kind == "f":
            ng, nr = np.isnan(g), np.isnan(r)
            np.testing.assert_array_equal(ng, nr, err_msg=f"{what}: {k} (NaN positions)")
            np.testing.assert_array_equal(bits(g)[~ng], bits(r)[~nr], err_msg=f"{what}: {k}")
        else:
            np.testing.assert_array_equal(g, r, err_msg=f"{what}: {k}")


# ---- 1. done patterns ------------------------------------------------------------------------------------
_r5 = np.random.default_rng(505)
PATTERNS = {
    "none+all": ([], list(range(64))),
    "first+last": ([0], [63]),
    "group+partial": ([0, 1, 2], [5, 17, 33, 60]),
    "first22+alternate": (list(range(22)), list(range(0, 64, 2))),
    "random5": (sorted(_r5.choice(64, 5, replace=False).tolist()), sorted(_r5.choice(64, 5, replace=False).tolist())),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_done_patterns(monkeypatch, precision, pattern):
    """E = 128 (two blocks), one auto-reset step; step_counter = 1928 (>= the 1921 of the 8 s limit) makes
    the chosen lanes done, the others start well inside every limit (tilt 0.2 rad against 0.4, |x|, |y| <=
    0.5 against 1.5, z <= 1.3 against 2).  Both staged kernels against the reference; the terminal rows of
    the envs that are not done still hold the sentinel."""
    E = 128
    rng = np.random.default_rng(71)
    real = np.float64 if precision == "fp64" else np.float32
    env, orc = pair(E, Physics.PYB, precision=precision, autoreset=True, seed=5, initial_xyzs=[0, 0, 1.0], init_noise=BENCH_NOISE)
    env.reset()
    f, i = random_states(rng, E, env, orc, tilt=0.2)
    env.close()
    f = f.astype(real)
    _, inames = orc.field_names()
    i[inames.index("ring_head")] = 7
    want = np.zeros(E, bool)
    b0, b1 = PATTERNS[pattern]
    want[b0] = True
    want[[64 + l for l in b1]] = True
    i[inames.index("step_counter")][want] = 1928
    act = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    env = make_env(monkeypatch, E, precision, REFERENCE)
    ref = step_once(env, f, i, act)
    env.close()
    done = ref["term"] | ref["trunc"]
    np.testing.assert_array_equal(done, want)
    assert (ref["tobs"][~done] == SENTINEL).all() and not (ref["tobs"][done] == SENTINEL).any()
    for name, sw in STAGED.items():
        env = make_env(monkeypatch, E, precision, sw)
        got = step_once(env, f, i, act)
        env.close()
        assert_same_bits(got, ref, f"{name}, {pattern}")
        assert (got["tobs"][~done] == SENTINEL).all()


# ---- 2. free run -----------------------------------------------------------------------------------------
def free_run(monkeypatch, E, T, acts, precision, switches):
    env = make_env(monkeypatch, E, precision, switches, seed=99)
    env._tobs.fill_(SENTINEL)
    seq = [outputs(env, env.step(acts[t].to(env.device))) for t in range(T)]
    env.close()
    return seq


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_free_run(monkeypatch, precision):
    """60 auto-reset steps at E = 128 from bench.py's start distribution with seeded U[-1, 1] actions: each
    staged kernel against the reference at every step, in everything a step gives and leaves (a terminal row
    keeps what its env's last done step wrote, or the sentinel).  The run must hold a step with three or
    more done envs in one block and a step with a block that has none.  (It also holds blocks with more
    than twelve, a second pass of the helper waves' copy; test_done_patterns has 22, 32 and 64.)"""
    E, T = 128, 60
    acts = torch.from_numpy(np.random.default_rng(99).uniform(-1, 1, (T, E, 1, 4)).astype(np.float32))
    ref = free_run(monkeypatch, E, T, acts, precision, REFERENCE)
    per_block = np.array([(r["term"] | r["trunc"]).reshape(E // 64, 64).sum(1) for r in ref])
    print("done envs per step and block:", per_block.tolist())
    assert (per_block >= 3).any() and (per_block == 0).any()
    for name, sw in STAGED.items():
        got = free_run(monkeypatch, E, T, acts, precision, sw)
        ever = np.zeros(E, bool)
        for t in range(T):
            assert_same_bits(got[t], ref[t], f"{name}, step {t}")
            ever |= ref[t]["term"] | ref[t]["trunc"]
            assert (got[t]["tobs"][~ever] == SENTINEL).all(), f"{name}, step {t}"


# ---- 3. angle edges --------------------------------------------------------------------------------------
SCAN = 12   # cases either side of asin(0.99999), one ulp of sarg apart


def ulp_steps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def edge_quaternions():
    """(name, quaternion xyzw) of the attitudes at which the angle forms take another path"""
    out = [("identity", np.array([0.0, 0.0, 0.0, 1.0])), ("nan", np.full(4, np.nan))]
    # |sarg| around 0.99999: a pure pitch by th has sarg = sin th, and near asin(0.99999) one ulp of sarg
    # (1.1e-16) is 2.5e-14 of th (cos th = 4.5e-3; a step of one ulp in the quaternion moves sarg by a
    # hundredth of an ulp).  The scan walks th by that much per case, so where the kernel's own sarg (which
    # carries an ulp of rounding noise from the normalisation and the product) crosses the threshold the
    # neighbouring cases lie an ulp or two either side of it; test_angle_edges checks that it does cross
    for sign in (1.0, -1.0):
        for k in range(-SCAN, SCAN + 1):
            th = np.arcsin(0.99999) + k * 2.5e-14
            out.append((f"sarg{'+' if sign > 0 else '-'}0.99999 {k:+d}", np.array([0.0, sign * np.sin(th / 2), 0.0, np.cos(th / 2)])))
    # roll and yaw at the seams and the octant joints of atan2
    marks = [0.0, np.pi / 4, -np.pi / 4, np.pi / 2, -np.pi / 2, np.pi - 1e-12, -(np.pi - 1e-12)]
    for a in marks:
        out.append((f"roll {a:+.4f}", np.asarray(O.quat_from_euler(np.array([a, 0.05, 0.3])))))
        out.append((f"yaw {a:+.4f}", np.asarray(O.quat_from_euler(np.array([0.1, -0.05, a])))))
        out.append((f"roll = yaw {a:+.4f}", np.asarray(O.quat_from_euler(np.array([a, 0.0, a])))))
    # min / max around tan(pi/8): a pure roll (x, 0, 0, w) by a has min / max = tan a (a = pi/8) or cot a
    # (a = 3 pi/8), a pure yaw (0, 0, z, w) likewise; x (z) stepped one ulp at a time moves the ratio by
    # about an ulp per step across the comparison with tan(pi/8)
    for axis in (0, 2):
        for a in (np.pi / 8, 3 * np.pi / 8, -np.pi / 8, -3 * np.pi / 8, 5 * np.pi / 8, 7 * np.pi / 8):
            s, c = np.sin(a / 2), np.cos(a / 2)
            for k in range(-4, 5):
                q = np.array([0.0, 0.0, 0.0, c])
                q[axis] = ulp_steps(s, k)
                out.append((f"{'roll' if axis == 0 else 'yaw'} {a:+.4f} {k:+d} ulp", q))
    return out


def edge_state(names, inames, nf, ni, quats, rng):
    """E = len(quats) hovering envs with the given attitudes: zero velocity and zero omega, so that equal
    RPMs (no torque) keep the attitude through the step"""
    E = len(quats)
    idx = {n: k for k, n in enumerate(names)}
    f = np.zeros((nf, E))
    i = np.zeros((ni, E), np.int32)
    f[idx["pos_z"]] = 1.0
    for k, ax in enumerate("xyzw"):
        f[idx[f"quat_{ax}"]] = quats[:, k]
        f[idx[f"link_quat_{ax}"]] = quats[:, k]
    ring = [k for k, n in enumerate(names) if n.startswith("ring_")]
    f[ring] = rng.uniform(-1, 1, (len(ring), E)).astype(np.float32)
    i[inames.index("ring_head")] = 7
    i[inames.index("episode")] = 1
    return f, i


def test_angle_edges(monkeypatch):
    """fp64, E = 64 (one chain wave and its helper waves).  Each edge attitude once in all 64 lanes, and once
    in one lane (which lane moves with the case) among 63 benign attitudes: both against the reference, and
    in the mixed wave the 63 others must have the bits they have in the all-benign wave, whichever form
    the edge lane's vote sent the wave to."""
    E = 64
    rng = np.random.default_rng(8)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    env = make_env(monkeypatch, E, "fp64", {})
    names, inames = env.state_field_names()
    f0, i0 = env.get_state()
    nf, ni = f0.shape[0], i0.shape[0]
    act = np.full((E, 1, 4), 0.1, np.float32)
    benign = np.array([O.quat_from_euler(r) for r in rng.uniform(-0.1, 0.1, (E, 3))])
    fb, ib = edge_state(names, inames, nf, ni, benign, rng)
    base = step_once(env, fb, ib, act)
    assert_same_bits(base, step_once(ref_env, fb, ib, act), "benign wave")
    assert not np.isnan(base["obs"]).any()
    edges = edge_quaternions()
    gimbal = {}
    for n, (name, q) in enumerate(edges):
        fu, iu = fb.copy(), ib.copy()
        for k, ax in enumerate("xyzw"):
            fu[names.index(f"quat_{ax}")] = q[k]
            fu[names.index(f"link_quat_{ax}")] = q[k]
        ref = step_once(ref_env, fu, iu, act)
        assert_same_bits(step_once(env, fu, iu, act), ref, f"uniform wave, {name}")
        gimbal[name] = abs(ref["tobs"][0, 4]) == np.float32(np.pi / 2) if (ref["term"] | ref["trunc"])[0] else False
        lane = (7 * n + 3) % E
        fm, im = fb.copy(), ib.copy()
        for k, ax in enumerate("xyzw"):
            fm[names.index(f"quat_{ax}"), lane] = q[k]
            fm[names.index(f"link_quat_{ax}"), lane] = q[k]
        got = step_once(env, fm, im, act)
        assert_same_bits(got, step_once(ref_env, fm, im, act), f"mixed wave, {name} in lane {lane}")
        others = np.arange(E) != lane
        assert_same_bits(got, base, f"mixed wave, {name}: the other lanes", rows=others)
    # the scans did cross the gimbal threshold: asin below it, exactly +-pi/2 from it on
    for sign in "+-":
        scan = [bool(gimbal[f"sarg{sign}0.99999 {k:+d}"]) for k in range(-SCAN, SCAN + 1)]
        print(f"gimbal branch along the sarg {sign}0.99999 scan:", "".join("G" if g else "." for g in scan))
        assert not scan[0] and scan[-1], scan
    env.close()
    ref_env.close()
