"""The end of the chain wave in the fp64 hover step with angle helper waves ("Chain end"): the
chain decides |roll| > 0.4 || |pitch| > 0.4 from the quaternion (|sarg| against sin 0.4, |y0| against
tan 0.4 x0) and runs from barrier A into its state stores without waiting for an angle; the helper waves put
the float32 angles into the staged rows, copy out all eighteen columns, take the obs of done rows from the
reset helper's block and move whole terminal rows.  A lane within a relative band of BAND of a threshold (or
with x0 <= 0, gimbal lock, a NaN) sends its whole wave down the earlier path, which tests the angles.  No
value changes: every case is held, bit for bit, to the row-store kernel without helper waves
(ADRP_STAGE_ROWS=0, ADRP_RESET_HELPER=0).
Needs an MI355X: -m gpu.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gym_pybullet_adrp_amd.utils.enums import Physics  # noqa: E402
from oracle import oracle as O  # noqa: E402

from test_hover_gpu import pair, random_states  # noqa: E402
from test_hover_tail_gpu import (BENCH_NOISE, PATTERNS, REFERENCE, SENTINEL, assert_same_bits, edge_state,  # noqa: E402
                                 make_env, outputs, step_once)

BAND = 1e-9      # kTruncBand (csrc/adrp_device.h): relative half-width of the unsure band around a threshold
LIMIT = 0.4      # HoverAviary._computeTruncated's tilt limit
FAR = [s * d for d in (1e-3, 1e-2, 0.1) for s in (1, -1)]
INSIDE = [0.0] + [s * d for d in (1e-15, 1e-12, 1e-10) for s in (1, -1)]
NEAR = [s * d for d in (3e-9, 1e-8, 1e-7, 1e-6) for s in (1, -1)]


def rel_distance(axis, delta):
    """relative distance of the quaternion form's left side from its threshold at a tilt of LIMIT + delta"""
    fn = np.tan if axis == "roll" else np.sin
    return abs(fn(LIMIT + delta) / fn(LIMIT) - 1.0)


def tilt_cases(deltas):
    """(axis, roll, pitch) with the axis' angle at +-(LIMIT + delta) and the other at 0.1"""
    out = []
    for axis in ("roll", "pitch"):
        for sign in (1.0, -1.0):
            for d in deltas:
                a = sign * (LIMIT + d)
                out.append((axis, a, 0.1) if axis == "roll" else (axis, 0.1, a))
    return out


def fill(cases, filler, n=64):
    return cases + [filler[k % len(filler)] for k in range(n - len(cases))]


def still_state(env, lanes, rng):
    """hovering envs with the given (roll, pitch): zero velocity and omega, so equal RPMs keep the attitude"""
    names, inames = env.state_field_names()
    f0, i0 = env.get_state()
    quats = np.array([O.quat_from_euler(np.array([r, p, 0.0])) for _, r, p in lanes], dtype=np.float64)
    return edge_state(names, inames, f0.shape[0], i0.shape[0], quats, rng)


def test_threshold_straddle(monkeypatch):
    """E = 192, one step, the attitude fixed through the step.  Block 0: tilts far from the limit (the chain's
    fast path); block 1: tilts inside the band, a roll of 2.0 (x0 < 0) and a pitch of 1.5 among far lanes (the
    fall-back); block 2: tilts just outside the band (the fast path next to the threshold)."""
    assert all(rel_distance(ax, d) > BAND for ax in ("roll", "pitch") for d in NEAR + FAR)
    assert all(rel_distance(ax, d) < BAND for ax in ("roll", "pitch") for d in INSIDE)
    far, near = tilt_cases(FAR), tilt_cases(NEAR)
    blocks = [fill(far, far), fill(tilt_cases(INSIDE) + [("roll", 2.0, 0.1), ("pitch", 0.1, 1.5)], far), fill(near, near)]
    lanes = [c for b in blocks for c in b]
    E = len(lanes)
    assert E == 192
    rng = np.random.default_rng(12)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    env = make_env(monkeypatch, E, "fp64", {})
    f, i = still_state(env, lanes, rng)
    act = np.full((E, 1, 4), 0.1, np.float32)
    ref = step_once(ref_env, f, i, act)
    got = step_once(env, f, i, act)
    env.close()
    ref_env.close()
    # on the reference's flags: every block holds truncated and not truncated lanes for roll and for pitch
    for b in range(3):
        for axis in ("roll", "pitch"):
            flags = [bool(ref["trunc"][64 * b + l]) for l in range(64) if lanes[64 * b + l][0] == axis]
            print(f"block {b} {axis}: {sum(flags)} of {len(flags)} truncated")
            assert any(flags) and not all(flags), (b, axis)
    assert_same_bits(got, ref, "threshold straddle")


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_done_rows_from_helpers(monkeypatch, pattern):
    """E = 128, one auto-reset step per ring head in {0, 7, 14}, test_hover_tail_gpu's done patterns (step_counter
    = 1928 makes the chosen lanes done).  In group+partial done lane 2 of block 0 starts at a roll of 2.0: x0 < 0,
    an unsure lane, so that block's chain takes the fall-back with done lanes.  With the terminal rows present
    and absent (the handle bound without them)."""
    E = 128
    rng = np.random.default_rng(71)
    env0, orc = pair(E, Physics.PYB, precision="fp64", autoreset=True, seed=5, initial_xyzs=[0, 0, 1.0], init_noise=BENCH_NOISE)
    env0.reset()
    f, i = random_states(rng, E, env0, orc, tilt=0.2)
    env0.close()
    names, inames = orc.field_names()
    want = np.zeros(E, bool)
    b0, b1 = PATTERNS[pattern]
    want[b0] = True
    want[[64 + l for l in b1]] = True
    i[inames.index("step_counter")][want] = 1928
    if pattern == "group+partial":
        q = np.asarray(O.quat_from_euler(np.array([2.0, 0.1, 0.3])))
        for k, ax in enumerate("xyzw"):
            f[names.index(f"quat_{ax}"), 2] = q[k]
            f[names.index(f"link_quat_{ax}"), 2] = q[k]
    act = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    env = make_env(monkeypatch, E, "fp64", {})
    bare = make_env(monkeypatch, E, "fp64", {})
    bare.h.bind(bare._obs, bare._rew, bare._term, bare._trunc, None)   # no terminal rows
    for head in (0, 7, 14):
        i[inames.index("ring_head")] = head
        ref = step_once(ref_env, f, i, act)
        done = ref["term"] | ref["trunc"]
        np.testing.assert_array_equal(done, want)
        assert (ref["tobs"][~done] == SENTINEL).all() and not (ref["tobs"][done] == SENTINEL).any()
        got = step_once(env, f, i, act)
        assert_same_bits(got, ref, f"{pattern}, head {head}")
        assert (got["tobs"][~done] == SENTINEL).all()
        # obs rows of done envs hold the reset obs: the state the step left, in float32
        for k, n in enumerate(("pos_x", "pos_y", "pos_z")):
            np.testing.assert_array_equal(got["obs"][done, k], got["f"][names.index(n)][done].astype(np.float32))
        none = step_once(bare, f, i, act)
        assert (none["tobs"] == SENTINEL).all()
        none["tobs"] = ref["tobs"]
        assert_same_bits(none, ref, f"{pattern}, head {head}, no terminal rows")
    for e in (ref_env, env, bare):
        e.close()


@pytest.mark.parametrize("E", [64, 128])
def test_free_run(monkeypatch, E):
    """40 auto-reset steps from bench.py's start distribution with seeded U[-1, 1] actions, every step against
    the reference; the run holds done envs."""
    T = 40
    acts = torch.from_numpy(np.random.default_rng(99).uniform(-1, 1, (T, E, 1, 4)).astype(np.float32))
    seqs = []
    for sw in (REFERENCE, {}):
        env = make_env(monkeypatch, E, "fp64", sw, seed=99)
        env._tobs.fill_(SENTINEL)
        seqs.append([outputs(env, env.step(acts[t].to(env.device))) for t in range(T)])
        env.close()
    ref, got = seqs
    per_step = [int((r["term"] | r["trunc"]).sum()) for r in ref]
    print("done envs per step:", per_step)
    assert sum(per_step) >= 1
    for t in range(T):
        assert_same_bits(got[t], ref[t], f"E {E}, step {t}")


def test_nan_and_gimbal_lanes(monkeypatch):
    """E = 64: one lane with a NaN quaternion component and one at a pitch of pi/2 - 1e-7 (gimbal lock) among
    ordinary lanes.  Equal to the reference (a NaN is a NaN in both), and the ordinary lanes have the bits they
    have in the all-ordinary wave, whichever path the vote sent the chain to."""
    E = 64
    rng = np.random.default_rng(8)
    ref_env = make_env(monkeypatch, E, "fp64", REFERENCE)
    env = make_env(monkeypatch, E, "fp64", {})
    names, inames = env.state_field_names()
    f0, i0 = env.get_state()
    benign = np.array([O.quat_from_euler(r) for r in rng.uniform(-0.1, 0.1, (E, 3))])
    fb, ib = edge_state(names, inames, f0.shape[0], i0.shape[0], benign, rng)
    act = np.full((E, 1, 4), 0.1, np.float32)
    base = step_once(env, fb, ib, act)
    assert_same_bits(base, step_once(ref_env, fb, ib, act), "ordinary wave")
    assert not np.isnan(base["obs"]).any()
    fm, im = fb.copy(), ib.copy()
    fm[names.index("quat_y"), 11] = np.nan
    q = np.asarray(O.quat_from_euler(np.array([0.0, np.pi / 2 - 1e-7, 0.0])))
    for k, ax in enumerate("xyzw"):
        fm[names.index(f"quat_{ax}"), 42] = q[k]
        fm[names.index(f"link_quat_{ax}"), 42] = q[k]
    ref = step_once(ref_env, fm, im, act)
    got = step_once(env, fm, im, act)
    env.close()
    ref_env.close()
    assert np.isnan(ref["tobs"][11]).any() or np.isnan(ref["obs"][11]).any() or np.isnan(ref["f"][:, 11]).any()
    assert ref["trunc"][42]
    assert_same_bits(got, ref, "NaN and gimbal lanes")
    others = np.ones(E, bool)
    others[[11, 42]] = False
    assert_same_bits(got, base, "the ordinary lanes", rows=others)
