"""The pose hand-off of the fp64 hover step with a translation wave ("Pose hand-off"): the chain
wave hands the quaternion of each of its poses through LDS slots (s + 2: the pose behind sub-step s; slots 0 and 1,
the cached link basis and the pose at entry, are state fields that the translation wave loads itself) and no longer
forms their z axes; the translation wave forms them from the quaternions with the chain's own expression
(col2_fm), for the thrust axis (slot s with the link lag, s + 1 without) and for the plane contact test (slot
s + 2).  The expression and its inputs are the chain's, so no
value changes: every case is held, bit for bit, to the row-store kernel without helper waves
(ADRP_STAGE_ROWS=0, ADRP_RESET_HELPER=0) in all five outputs, the terminal rows and the whole state.
Needs an MI355X: -m gpu.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.envs.hover import HoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Physics  # noqa: E402
from oracle import oracle as O  # noqa: E402

from test_hover_gpu import pair  # noqa: E402,F401  (the helpers below build on it)
from test_hover_tail_gpu import BENCH_NOISE, REFERENCE, SENTINEL, assert_same_bits, make_env, outputs, step_once  # noqa: E402
from test_hover_transwave_gpu import KERNEL, contact_state, first_contact_substep, set_pose, start_states  # noqa: E402

GENERIC = "hover_step<f64,PYB,A4,B15,generic>"   # link_frame_lag off: the constants are not the compiled-in ones


# ---- 1. slot order -----------------------------------------------------------------------------------------
def spinning_states(E, seed):
    """start_states with every lane turning at 20 to 90 rad/s about an axis in the body's xy plane (and a little
    about z): the z axis turns by 0.08 to 0.375 rad per sub-step, so the thrust axis of slot k - 1 or k + 1 in
    place of slot k moves vel and pos far above their low-order bits"""
    f, i, orc, names, inames = start_states(E, seed)
    rng = np.random.default_rng(seed + 1)
    mag = rng.uniform(20.0, 90.0, E)
    phi = rng.uniform(0.0, 2 * np.pi, E)
    wz = rng.uniform(-2.0, 2.0, E)
    for l in range(E):
        set_pose(f, names, l, omega=(mag[l] * np.cos(phi[l]), mag[l] * np.sin(phi[l]), wz[l]))
    return f, i, names, inames


def final_vel32(o):
    """the step's final velocity per env as the obs row holds it (a done env's row is its terminal row)"""
    done = (o["term"] | o["trunc"])[:, None]
    return np.where(done, o["tobs"][:, 6:9], o["obs"][:, 6:9])


@pytest.mark.parametrize("E", [64, 192])
def test_slot_order(monkeypatch, E):
    """One block and three, link lag on (thrust axis from slot s; the kernel with the hand-off) and off (slot
    s + 1; the generic kernel): one auto-reset step from the spinning states, then eight free steps, unequal
    RPMs throughout, each step against the reference.  The two lag settings differ by exactly one slot, so their
    references must differ in every lane's velocity: that is the sensitivity the comparison relies on."""
    f, i, names, inames = spinning_states(E, 300 + E)
    acts = np.random.default_rng(E + 7).uniform(-1, 1, (9, E, 1, 4)).astype(np.float32)
    first = {}
    for lag in (True, False):
        seqs = []
        for sw in (REFERENCE, {}):
            env = make_env(monkeypatch, E, "fp64", sw, link_frame_lag=lag)
            assert env.kernel_name == (KERNEL["fp64"] if lag else GENERIC)
            seq = [step_once(env, f, i, acts[0])]
            seq += [outputs(env, env.step(torch.from_numpy(acts[t]).to(env.device))) for t in range(1, 9)]
            env.close()
            seqs.append(seq)
        for t in range(9):
            assert_same_bits(seqs[1][t], seqs[0][t], f"E {E}, lag {lag}, step {t}")
        first[lag] = seqs[0][0]
    moved = (final_vel32(first[True]) != final_vel32(first[False])).any(axis=1)
    assert moved.all(), f"lanes whose velocity does not depend on the slot: {np.flatnonzero(~moved).tolist()}"


# ---- 2. contact through the new pose path ------------------------------------------------------------------
def test_contact_pose_path(monkeypatch):
    """test_hover_transwave_gpu's contact states (E = 128: first-sub-step contact, the crossing between
    sub-steps 7 and 8 that reads the last slot, tilted mid-step contact, lanes inside the guard without contact,
    one near-plane lane in a wave that otherwise flies high): the contact test now takes its z axis from the
    quaternion of slot s + 2.  Everything, the contact counter included, against the reference; the oracle
    confirms the last-slot lanes first."""
    E = 128
    rng = np.random.default_rng(3)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    env = make_env(monkeypatch, E, "fp64", {})
    assert env.kernel_name == KERNEL["fp64"] == ref_env.kernel_name
    names, inames = env.state_field_names()
    f0, i0 = env.get_state()
    f, i, specs = contact_state(names, inames, f0.shape[0], i0.shape[0], rng)
    act = rng.uniform(-0.2, 0.2, (E, 1, 4)).astype(np.float32)
    first = first_contact_substep(env.cfg, f, i, act)
    for w in range(2):
        lanes = first[64 * w:64 * w + 64]
        assert (lanes == 1).any() and (lanes == 8).any() and (lanes == 0).any(), (w, lanes.tolist())
    counts, res = [], []
    for e_ in (ref_env, env):
        e_.h.set_diagnostics(True)
        e_.h.contact_count(reset=True)
        res.append(step_once(e_, f, i, act))
        torch.cuda.synchronize()
        counts.append(e_.h.contact_count())
        e_.close()
    print("contact count: reference", counts[0], "pose hand-off", counts[1], "oracle", int((first > 0).sum()))
    assert counts[0] == int((first > 0).sum()) and counts[1] == counts[0]
    assert_same_bits(res[1], res[0], "ground contact")


# ---- 3. clamp and odd lanes --------------------------------------------------------------------------------
FAST, NAN_Q, GIMBAL = 21, 38, 55   # lanes


def test_clamp_and_odd_lanes(monkeypatch):
    """E = 64, one wave.  (a) one lane at |omega| = 250 rad/s among slow lanes: the wave-uniform clamp branch is
    taken and the quaternion handed out is the one committed behind it; (b) one lane whose quaternion is NaN and
    one at gimbal lock (pitch pi/2 - 1e-7).  The wave finishes, everything equals the reference, and the other
    lanes have the bits they have in the all-ordinary wave."""
    E = 64
    f, i, orc, names, inames = start_states(E, 23)
    act = np.random.default_rng(9).uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    env = make_env(monkeypatch, E, "fp64", {})
    assert env.kernel_name == KERNEL["fp64"]
    base = step_once(env, f, i, act)
    assert_same_bits(base, step_once(ref_env, f, i, act), "ordinary wave")
    # (a)
    fa = f.copy()
    set_pose(fa, names, FAST, omega=(250.0 / np.sqrt(3.0),) * 3)
    ref = step_once(ref_env, fa, i, act)
    got = step_once(env, fa, i, act)
    assert_same_bits(got, ref, "one fast lane")
    assert ref["trunc"][FAST] and np.abs(ref["tobs"][FAST, 9:12]).max() <= 100.0, ref["tobs"][FAST, 9:12]
    others = np.arange(E) != FAST
    assert_same_bits(got, base, "one fast lane: the slow lanes", rows=others)
    # (b)
    fb = f.copy()
    for ax in "xyzw":
        fb[names.index(f"quat_{ax}"), NAN_Q] = np.nan
        fb[names.index(f"link_quat_{ax}"), NAN_Q] = np.nan
    set_pose(fb, names, GIMBAL, rpy=(0.0, np.pi / 2 - 1e-7, 0.0), omega=(0.0, 0.0, 0.0))
    actb = act.copy()
    actb[GIMBAL] = 0.1                                       # equal RPMs: no torque, the attitude stays at the lock
    ref = step_once(ref_env, fb, i, actb)
    got = step_once(env, fb, i, actb)
    assert_same_bits(got, ref, "NaN and gimbal-lock lanes")
    assert np.isnan(ref["tobs"][NAN_Q]).any() or np.isnan(ref["f"][:, NAN_Q]).any() or ref["trunc"][NAN_Q]
    assert abs(ref["tobs"][GIMBAL, 4]) == np.float32(np.pi / 2), ref["tobs"][GIMBAL, 3:6]
    others = np.ones(E, bool)
    others[[NAN_Q, GIMBAL]] = False
    assert_same_bits(got, base, "NaN and gimbal-lock lanes: the other lanes", rows=others)
    env.close()
    ref_env.close()


# ---- 4. dirty LDS ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 192])
def test_dirty_lds(monkeypatch, E):
    """LDS keeps what the last workgroup on the CU left, mark words included.  Between two fp64 steps an fp32
    HoverAviary of 16,384 envs (256 workgroups: every CU; another LDS layout, rows and reset states where the
    fp64 kernel keeps its slots and marks) steps three times on the same device.  Both fp64 steps against the
    reference."""
    f, i, names, inames = spinning_states(E, 500 + E)
    acts = np.random.default_rng(E + 3).uniform(-1, 1, (2, E, 1, 4)).astype(np.float32)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    ref = [step_once(ref_env, f, i, acts[0]), outputs(ref_env, ref_env.step(torch.from_numpy(acts[1]).to(ref_env.device)))]
    ref_env.close()
    env = make_env(monkeypatch, E, "fp64", {})
    assert env.kernel_name == KERNEL["fp64"]
    other = HoverAviary(physics=Physics.PYB, precision="fp32", num_envs=16384, seed=7, initial_xyzs=[0, 0, 1.0],
                        init_noise=BENCH_NOISE)
    assert other.kernel_name == KERNEL["fp32"]
    other.reset()
    oact = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (16384, 1, 4)).astype(np.float32)).to(other.device)
    got = [step_once(env, f, i, acts[0])]
    for _ in range(3):
        other.step(oact)
    torch.cuda.synchronize()
    got.append(outputs(env, env.step(torch.from_numpy(acts[1]).to(env.device))))
    other.close()
    env.close()
    for t in range(2):
        assert_same_bits(got[t], ref[t], f"E {E}, step {t}")


# ---- 5. graph replay ---------------------------------------------------------------------------------------
def test_graph_replay(monkeypatch):
    """E = 64: eight steps captured in one graph and replayed give what the same eight steps launched one by one
    give, bit for bit: the four outputs and the terminal rows behind every step, and the state at the end."""
    E, T = 64, 8
    f, i, names, inames = spinning_states(E, 77)
    acts = np.random.default_rng(12).uniform(-1, 1, (T, E, 1, 4)).astype(np.float32)
    bufs = ("_obs", "_rew", "_term", "_trunc", "_tobs")
    runs = []
    for graphed in (False, True):
        env = make_env(monkeypatch, E, "fp64", {})
        assert env.kernel_name == KERNEL["fp64"]
        dacts = torch.from_numpy(acts).to(env.device)
        env.step(dacts[0])                                   # eager warm-up: the kernel is loaded before the capture
        torch.cuda.synchronize()
        env.set_state(torch.from_numpy(f), torch.from_numpy(i))
        env._tobs.fill_(SENTINEL)
        torch.cuda.synchronize()
        per_step = []

        def roll():
            for t in range(T):
                env.step(dacts[t])
                per_step.append([getattr(env, b).clone() for b in bufs])

        if graphed:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    roll()
            g.replay()
        else:
            roll()
        torch.cuda.synchronize()
        fs, is_ = env.get_state()
        runs.append(([[x.cpu().numpy().copy() for x in st] for st in per_step], fs.cpu().numpy().copy(), is_.cpu().numpy().copy()))
        env.close()
    (eager, fe, ie), (replayed, fg, ig) = runs

    def same(a, b, what):
        if a.dtype.kind == "f":
            na, nb = np.isnan(a), np.isnan(b)
            np.testing.assert_array_equal(na, nb, err_msg=what)
            a, b = np.where(na, 0, a), np.where(nb, 0, b)
            a = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
            b = b.view({4: np.uint32, 8: np.uint64}[b.dtype.itemsize])
        np.testing.assert_array_equal(a, b, err_msg=what)

    for t in range(T):
        for name, a, b in zip(bufs, replayed[t], eager[t]):
            same(a, b, f"step {t}: {name}")
    same(fg, fe, "state")
    same(ig, ie, "int state")
    assert not (eager[T - 1][4] == SENTINEL).all()           # some env was done: terminal rows were written
