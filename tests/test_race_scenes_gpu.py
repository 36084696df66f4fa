"""The race kernels' geometry decisions at constructed poses vs the CPU oracle.  Needs an MI355X: -m gpu.

tests/race_scenes.py puts every drone of a few hundred a known distance (measured by the oracle on
its post-step state) from one of the step's thresholds: the 0.45 m range, the 1e-6 m contact with
gate / obstacle parts, the plane and other drones, the gate rays, |omega| = 20, the bounds.  No drone
is within the bar of a threshold (fp32 1e-4 m, fp64 1e-9 m; tests/test_race_scenes.py proves that on
the CPU), so nothing is exempted here: after one env.step (two for `fin`) from the same
float32-representable state, gate, flags, the in-range flags, the current-gate column, terminated and
truncated equal the oracle's for every drone, in the four kernel variants (fp32 / fp64, four lanes
per drone / one), with the support-function bounds on and off for the scenes that reach them, and
once without the helper waves.  The dense scene loads a wave's pooled GJK queue (track_gjk_pool)
with more than 64 jobs, from envs with different tracks: several dealing rounds, the padding of the
last one, and jobs run by lanes of other envs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import race_scenes as RS  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import RaceMode  # noqa: E402
from oracle import oracle as O  # noqa: E402

VARIANTS = [("fp32", "1"), ("fp32", "0"), ("fp64", "1"), ("fp64", "0")]      # (precision, ADRP_RACE_QUAD)
VARIANT_IDS = ["fp32-quad", "fp32-lane", "fp64-quad", "fp64-lane"]
REFINED = [(s, c) for s, c in RS.SCENE_CONFIGS if s in ("range", "contact", "dense")]
BODY = [f"gate {g}" for g in range(4)] + [f"obstacle {k}" for k in range(4)]


def _where(sc, step, s, body=None):
    m = sc.margins[step]
    e, n = divmod(int(s), sc.N)
    txt = f"{sc.name}/{sc.config} class {sc.cls[s]!s} env {e} drone {n}"
    if body is not None:
        return txt + f" {BODY[body]}: oracle distance - 0.45 = {m['range'][s, body]:.3e}"
    causes = {"contact": m["contact"][s].min(), "plane": m["plane"][s], "pair": m["pair"][s].min(),
              "omega": m["omega"][s].max(), "bounds": m["bounds"][s].max()}
    return txt + f": oracle elimination margin {m['elim'][s]:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in causes.items())


def run_scene(monkeypatch, name, config, precision, quad, refine=None, helpers=None):
    monkeypatch.setenv("ADRP_RACE_QUAD", quad)
    if refine is not None:
        monkeypatch.setenv("ADRP_RACE_REFINE", refine)
    if helpers is not None:
        monkeypatch.setenv("ADRP_RACE_HELPERS", helpers)
    sc = RS.get_scene(name, config, precision == "fp64")
    level, N, physics, mode, E = RS.CONFIGS[config]
    env = MultiRaceAviary(level, num_drones=N, physics=physics, racemode=mode, num_envs=E, seed=RS.SEED,
                          autoreset=False, precision=precision, ctrl_freq=500)
    try:
        G = 2 if N <= 2 else 4 if N <= 4 else 8
        assert env.kernel_name == (f"race_step<{'f64' if precision == 'fp64' else 'f32'},{physics.name},G{G}"
                                   f"{',Q4' if quad == '1' else ''}>")
        env.h.set_diagnostics(True)
        orc = O.Oracle(env.cfg.copy())
        env.reset()
        orc.reset()
        names, inames = orc.field_names()
        assert env.state_field_names() == (names, inames)
        real = np.float64 if precision == "fp64" else np.float32
        act = torch.from_numpy(sc.act).to(env.device)
        f, i = sc.f, sc.i
        for step in range(sc.steps):
            f = RS.f32(f)
            orc.set_state(f, i)
            env.set_state(torch.from_numpy(f.astype(real)), torch.from_numpy(i))
            obs_o, _, te_o, tr_o, _ = orc.step(sc.act)
            obs_g, _, te_g, tr_g, _ = env.step(act)
            og = obs_g.cpu().numpy()
            ig = env.get_state()[1].cpu().numpy()
            f, i = orc.get_state()
            # this oracle and the generator's are the same: the margins belong to this step
            np.testing.assert_array_equal(i, sc.out[step]["i"])
            np.testing.assert_array_equal(obs_o, sc.out[step]["obs"])
            compare(sc, step, og, obs_o, ig, i, inames, te_g.cpu().numpy(), te_o, tr_g.cpu().numpy(), tr_o,
                    mode == RaceMode.COMPETE)
            # (adrp_diagnostic_contact_count is a counter of the hover kernels: the race step does not feed it)
    finally:
        env.close()


def compare(sc, step, og, obs_o, ig, io, inames, te_g, te_o, tr_g, tr_o, compete):
    N = sc.N
    err = []
    kg, kf = inames.index("gate"), inames.index("flags")
    for s in np.flatnonzero(ig[kg] != io[kg]):
        err.append(f"gate {ig[kg][s]} (oracle {io[kg][s]}): " + _where(sc, step, s))
    for s in np.flatnonzero(ig[kf] != io[kf]):
        err.append(f"flags {ig[kf][s]} (oracle {io[kf][s]}): " + _where(sc, step, s))
    for lo, off in ((28, 0), (44, 4)):
        for e, n, b in np.argwhere(og[..., lo:lo + 4] != obs_o[..., lo:lo + 4]):
            err.append(f"in-range flag {og[e, n, lo + b]:g} (oracle {obs_o[e, n, lo + b]:g}): " + _where(sc, step, e * N + n, off + b))
    for e, n in np.argwhere(og[..., 48] != obs_o[..., 48]):
        err.append(f"obs current gate {og[e, n, 48]:g} (oracle {obs_o[e, n, 48]:g}): " + _where(sc, step, e * N + n))
    for e in np.flatnonzero(te_g != te_o):
        err.append(f"terminated {te_g[e]} (oracle {te_o[e]}): {sc.name}/{sc.config} env {e} classes {list(sc.cls[e * N:(e + 1) * N])}")
    for e in np.flatnonzero(tr_g != tr_o):
        err.append(f"truncated {tr_g[e]} (oracle {tr_o[e]}): {sc.name}/{sc.config} env {e}")
    assert not err, f"step {step}: {len(err)} mismatches\n" + "\n".join(err[:12])
    # the gate / obstacle pose columns switch between actual and nominal with the flag
    np.testing.assert_allclose(og[..., 12:28], obs_o[..., 12:28], rtol=0, atol=1e-5)
    np.testing.assert_allclose(og[..., 32:44], obs_o[..., 32:44], rtol=0, atol=1e-5)
    np.testing.assert_allclose(og[..., :3], obs_o[..., :3], rtol=1e-4, atol=1e-4)
    if compete:
        np.testing.assert_allclose(og[..., 49:], obs_o[..., 49:], rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("precision,quad", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name,config", RS.SCENE_CONFIGS)
def test_scene(monkeypatch, name, config, precision, quad):
    run_scene(monkeypatch, name, config, precision, quad)


@pytest.mark.parametrize("precision,quad", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name,config", REFINED)
def test_scene_without_refined_bounds(monkeypatch, name, config, precision, quad):
    """ADRP_RACE_REFINE=0: the centre bounds alone queue every pair within the drone's bounding radius of
    a cut, so the GJK (and, in the dense scene, the pooled queue) decides what part_bounds_refined
    decides otherwise"""
    run_scene(monkeypatch, name, config, precision, quad, refine="0")


@pytest.mark.parametrize("name,config", [("dense", "level3"), ("contact", "level3"), ("gates", "level3")])
def test_scene_without_helper_waves(monkeypatch, name, config):
    """the one-lane fp32 kernel without its helper waves (ADRP_RACE_HELPERS=0: the track is read from
    global memory by T.lane(L, G, N, E) instead of the block's LDS copy)"""
    run_scene(monkeypatch, name, config, "fp32", "0", helpers="0")
