"""Cost of one wave's spline planning for the scripted racer: HardCodedCommander.replan on the host (scipy, one
splprep per distinct start, cold cache) against planner="device" (one adrp_race_plan launch), at level0,
E = 4,096, N = 2, from a fresh env.reset().

python tools/plan_time.py [--rounds 7] [--envs 4096] [--drones 2] [--starts reset|sample] [--out profiles/plan_time.json]

--starts reset (the default) plans from the reset observation as it is.  It carries the drones' NOMINAL start and
the nominal gates on every level, so the host's cache leaves N distinct fits per wave.  --starts sample writes the
E N distinct starts and gates of the tests' pinned sample (tests/plan_cases.py) into the rows: the cost of a wave
whose rows all differ, E N scipy fits on the host.

One process; a round resets the env, then runs each arm in turn (interleaved) on the same reset observation.
  host:   wall clock around replan() with an emptied cache (what every wave of simulate() pays: the starts of a
          new wave are new);
  device: wall clock around replan() (the launch, the status reduction and its one host read, which
          synchronises), and device events around the adrp_race_plan launch alone.
Medians over the rounds, spread = max - min.  The device arm is warmed up once before the rounds (the first launch
loads the code object).  Afterwards one simulate() wave with planner="device" gives the wave's step count, to set
the planning time against the wave's own stepping time (steps x the per-step cost of DESIGN.md 3.14).
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_pybullet_adrp_amd import _lib  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander  # noqa: E402
from gym_pybullet_adrp_amd.sim import simulate  # noqa: E402

STEP_US = 128.3      # one fused wave step at level0, E = 4,096, N = 2, both scripted


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "spread": float(v.max() - v.min()),
            "rounds": [float(x) for x in v]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--drones", type=int, default=2)
    ap.add_argument("--config", default="level0")
    ap.add_argument("--starts", default="reset", choices=("reset", "sample"))
    ap.add_argument("--no-host", action="store_true", help="skip the host arm (minutes with --starts sample)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("plan_time: no HIP device visible; nothing is measured without one")
    E, N = a.envs, a.drones
    env = MultiRaceAviary(a.config, num_drones=N, num_envs=E, seed=0, autoreset=False, precision="fp64", commands=True)
    rows = None
    if a.starts == "sample":
        from tests import plan_cases
        start, gates = plan_cases.sample(E * N)
        rows = torch.from_numpy(plan_cases.obs_rows(start, gates, width=28)).to(env.device).reshape(E, N, 28)

    def fresh_obs():
        obs, _ = env.reset()
        if rows is not None:
            obs[:, :, 0:2] = rows[:, :, 0:2]
            obs[:, :, 12:28] = rows[:, :, 12:28]
        return obs

    obs = fresh_obs()
    dev = HardCodedCommander(obs, planner="device")           # warm-up: the first launch
    host = None
    lib, stream = _lib.load(), _lib._raw_stream(env.device.index)
    t_host, t_dev, t_launch, diff, fallbacks = [], [], [], [], 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(a.rounds):
        obs = fresh_obs()
        torch.cuda.synchronize()
        if not a.no_host:
            if host is None:
                t0 = time.perf_counter()
                host = HardCodedCommander(obs)                # the constructor plans: a cold cache by construction
            else:
                host._cache.clear()
                t0 = time.perf_counter()
                host.replan(obs)
            torch.cuda.synchronize()
            t_host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        dev.replan(obs)
        t_dev.append(time.perf_counter() - t0)                # (replan ends on its host read)
        e0.record()
        rc = lib.adrp_race_plan(ctypes.byref(dev._plan_io), stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, lib.adrp_last_error(None).decode()
        t_launch.append(e0.elapsed_time(e1) * 1e-3)
        fallbacks = dev.host_fallbacks
        if host is not None:
            diff.append(float((dev.reference_trajectory - host.reference_trajectory).abs().max()))
        print(f"round {r}: host {t_host[-1] if t_host else float('nan'):.3f} s, device replan {t_dev[-1] * 1e3:.3f} ms, "
              f"launch {t_launch[-1] * 1e3:.3f} ms", flush=True)
    st = dev.plan_status.cpu().numpy()
    obs = obs.clone()
    env.close()
    res = simulate(a.config, "hardcoded", n_runs=E, n_drones=N, num_envs=E, planner="device", return_results=True)
    steps = int(res.episode_lengths.max())
    out = {"config": a.config, "starts": a.starts, "distinct_rows": int(torch.unique(obs.reshape(E * N, -1)[:, :28], dim=0).shape[0]),
           "num_envs": E, "num_drones": N, "rounds": a.rounds,
           "host_replan_s": stats(t_host) if t_host else None,
           "device_replan_s": stats(t_dev), "device_launch_s": stats(t_launch),
           "device_host_fallbacks": int(fallbacks),
           "knot_counts": {str(k): int(v) for k, v in zip(*np.unique((st >> 8) & 255, return_counts=True))},
           "max_abs_device_minus_host_m": max(diff) if diff else None,
           "wave_steps": steps, "step_us_design_3_14": STEP_US, "wave_stepping_s": steps * STEP_US * 1e-6,
           "device": torch.cuda.get_device_name(0)}
    out["device_replan_over_wave_stepping"] = out["device_replan_s"]["median"] / out["wave_stepping_s"]
    if t_host:
        out["host_replan_over_wave_stepping"] = out["host_replan_s"]["median"] / out["wave_stepping_s"]
        out["host_over_device"] = out["host_replan_s"]["median"] / out["device_replan_s"]["median"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
