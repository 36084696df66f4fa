"""Command-line twin of the reference's scripts/sim.py (``fire.Fire(simulate)``): evaluate the drones' controllers
over n_runs races, batched on the GPU (gym_pybullet_adrp_amd/sim.py).

python tools/sim.py --config level0 --controller hardcoded,zip:PATH --n_runs 4096 --n_drones 2 [--num_envs 4096]

--controller: one entry per drone, comma-separated, or a single entry used for all drones: ``hardcoded``
(HardCodedController), ``zip:PATH`` (an SB3 PPO zip driven as the RLController drives it; ``zip:PATH:absolute`` for
the RLControllerTwoGates transform) or ``none``.  ``--planner device`` plans the hardcoded drones' splines on the GPU
(one launch per wave) instead of with scipy on the host.  Prints the episode times (the reference's return value) and a
per-drone table: finish rate, mean finish time, elimination rate, wins.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gym_pybullet_adrp_amd.sim import simulate  # noqa: E402


def table(res):
    """per-drone rows (drone, finish rate, mean finish time [s] or nan, elimination rate, wins) of a RaceResults"""
    fin, elim, win, ft = res.finish_step >= 0, res.elim_step >= 0, res.winner, res.finish_times
    rows = []
    for n in range(fin.shape[1]):
        mean = float(np.nanmean(ft[:, n])) if fin[:, n].any() else float("nan")
        rows.append((n, float(fin[:, n].mean()), mean, float(elim[:, n].mean()), int((win == n).sum())))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="level0", help="preset name or YAML path (reference schema)")
    ap.add_argument("--controller", default="hardcoded", help="comma-separated: hardcoded | zip:PATH[:absolute] | none")
    ap.add_argument("--n_runs", type=int, default=10)
    ap.add_argument("--n_drones", type=int, default=2)
    ap.add_argument("--num_envs", type=int, default=None, help="races per wave (default min(n_runs, 4096))")
    ap.add_argument("--precision", default="fp64", choices=("fp32", "fp64"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--planner", default="host", choices=("host", "device"),
                    help="where the hardcoded controllers plan their splines: scipy on the host, or one launch per wave")
    ap.add_argument("--quiet", action="store_true", help="do not print the episode times")
    args = ap.parse_args(argv)
    controllers = [None if c.lower() == "none" else c for c in args.controller.split(",")]
    res = simulate(args.config, controllers, n_runs=args.n_runs, n_drones=args.n_drones, num_envs=args.num_envs,
                   precision=args.precision, seed=args.seed, return_results=True, planner=args.planner)
    if not args.quiet:
        print("episode times [s]:", " ".join(f"{t:.2f}" for t in res.episode_times))
    print(f"{args.n_runs} runs, mean episode time {res.episode_times.mean():.3f} s, "
          f"{int(res.terminated.sum())} terminated, {int(res.truncated.sum())} truncated")
    print(f"{'drone':>5} {'finished':>9} {'mean finish [s]':>16} {'eliminated':>11} {'wins':>6}")
    for n, fr, mt, er, w in table(res):
        print(f"{n:>5} {fr:>9.3f} {mt:>16.3f} {er:>11.3f} {w:>6}")
    print(f"{'-':>5} {'':>9} {'':>16} {'':>11} {int((res.winner < 0).sum()):>6}  (no finisher)")


if __name__ == "__main__":
    main()
