"""Per-drone PPO on a multi-drone race: tools/learn_hover.py's loop on MultiRaceAviary(COMPETE, autoreset=False).

python tools/learn_race.py [--envs 256] [--drones 4] [--n-steps 128] [--iterations 20] [--batch-size 1024]
                           [--n-epochs 10] [--seed 0] [--precision fp32] [--out FILE] [--save policy.pth]
                           [--roster learner,hardcoded[,snapshot,none]] [--snapshot-every 5] [--eval-runs 64]
                           [--end-on env|learners] [--target-kl K] [--learning-rate 3e-4] [--clip-range 0.2]
                           [--lr-schedule constant|linear] [--clip-schedule constant|linear]

Every drone is an agent of one shared policy (49 inputs: the drone's own state, the gates, the obstacles and the
gate id; four outputs, RLController's relative FULLSTATE setpoint); the reward is the RewardWrapper's, per drone.
Per iteration: MultiAgentRolloutCollector.collect() (n_steps env.steps of every env), PPOLearner.train() on the
valid samples (a drone that was eliminated or finished gives none until its env is reset), then one line with
episode_summary(): the mean return and length of the agent episodes that ended during the rollout (raw rewards,
without the time-limit bootstrap).  The reference cannot run this loop: its README lists training more than one
agent in MultiRaceAviary as a limitation of its sub-process controllers.  No learning bar is set here.

With --roster the drones race opponents (RosterRolloutCollector, one entry per drone: --drones is then the number of
entries): "learner" drones are samples of the policy being trained, "hardcoded" is the scripted HardCodedController,
"snapshot" a frozen copy of the learner (PPOLearner.snapshot(), refreshed every --snapshot-every rollouts: self-play)
and "none" an idle drone; the env runs in command mode.  --eval-runs R finishes with simulate() over R races, a
snapshot of the learner in the learner slots against the same opponents, and prints per-drone wins and finish rates.
--end-on learners (with --roster) resets an env with its last learner instead of with its race: against a scripted
racer the rollout's rows are then almost all valid (valid_fraction on every line).

--target-kl, --lr-schedule and --clip-schedule are tools/learn_hover.py's: SB3's early stop as a device latch
(stop_info on every line) and linear schedules over the run.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.rollout import MultiAgentRolloutCollector, RosterRolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.sim import simulate  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import RaceMode  # noqa: E402
from gym_pybullet_adrp_amd.ppo import PPOLearner  # noqa: E402
from tools.learn_hover import last_epoch_stats, rates, sb3_init  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--drones", type=int, default=4)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "fp64"))
    ap.add_argument("--out", default=None, help="JSON log of the run")
    ap.add_argument("--save", default=None, help="policy.pth-style file of the final parameters")
    ap.add_argument("--roster", default=None, help="comma-separated roles, one per drone: learner, hardcoded, snapshot, none")
    ap.add_argument("--snapshot-every", type=int, default=5, help="rollouts between refreshes of the snapshot opponents")
    ap.add_argument("--eval-runs", type=int, default=0, help="races of the closing simulate() table (with --roster)")
    ap.add_argument("--end-on", default="env", choices=("env", "learners"), help="with --roster: what ends an env")
    ap.add_argument("--target-kl", type=float, default=None, help="SB3's target_kl: stop a train() once approx_kl > 1.5 x this")
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--clip-range", type=float, default=0.2)
    ap.add_argument("--lr-schedule", default="constant", choices=("constant", "linear"), help="linear: to 0 at the end of the run")
    ap.add_argument("--clip-schedule", default="constant", choices=("constant", "linear"))
    args = ap.parse_args()
    if args.end_on != "env" and not args.roster:
        raise SystemExit("--end-on learners needs --roster: without one every drone is a learner and the env ends with the last")
    names = [r.strip().lower() for r in args.roster.split(",")] if args.roster else None
    if names:
        bad = [r for r in names if r not in ("learner", "hardcoded", "snapshot", "none")]
        if bad or "learner" not in names:
            raise SystemExit(f"--roster: entries are learner, hardcoded, snapshot, none, with at least one learner (got {names})")
        args.drones = len(names)
    env = MultiRaceAviary("level0", num_drones=args.drones, racemode=RaceMode.COMPETE, num_envs=args.envs, seed=args.seed,
                          precision=args.precision, autoreset=False, commands=bool(names))
    pol = DevicePolicy(sb3_init(49, 64, 4, args.seed), "tanh", 0, "relative")
    learner = PPOLearner(pol, n_epochs=args.n_epochs, batch_size=args.batch_size, seed=args.seed, **rates(args))
    learner.set_target_kl(args.target_kl)
    snaps = {}                       # drone -> its current frozen copy of the learner
    if names:
        snaps = {n: learner.snapshot() for n, r in enumerate(names) if r == "snapshot"}
        col = RosterRolloutCollector(env, pol, [snaps.get(n, None if r == "none" else r) for n, r in enumerate(names)],
                                     args.n_steps, seed=args.seed, end_on=args.end_on)
    else:
        col = MultiAgentRolloutCollector(env, pol, args.n_steps, seed=args.seed)
    col.reset()
    log, samples, t0 = [], 0, time.time()
    for it in range(args.iterations):
        if snaps and it and it % max(1, args.snapshot_every) == 0:
            for n, old in list(snaps.items()):
                snaps[n] = learner.snapshot()
                col.set_opponent(n, snaps[n])
                old.close()
        col.collect()
        stats = learner.train(col, progress_remaining=1.0 - it / args.iterations)
        valid = int(col.valid.sum())
        samples += valid
        s, stop = last_epoch_stats(learner, stats)
        rec = {"iteration": it, "valid_samples": samples, "valid_fraction": valid / (col.T * col.E),
               "policy_loss": s[0], "value_loss": s[1], "approx_kl": s[3], "clip_fraction": s[4],
               "wall_s": round(time.time() - t0, 3)}
        if stop is not None:
            rec["stop_info"] = stop
        rec.update(col.episode_summary())
        log.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"args": vars(args), "log": log}, f, indent=1)
            f.write("\n")
    if args.save:
        torch.save({k: v.cpu() for k, v in learner.state_dict().items()}, args.save)
    if names and args.eval_runs > 0:
        evaluate(names, learner, snaps, args)
    learner.close()
    for p in [pol] + list(snaps.values()):
        p.close()
    env.close()


def evaluate(names, learner, snaps, args):
    """the closing table: simulate() with a snapshot of the learner in the learner slots, the same opponents"""
    me = learner.snapshot()
    controllers = [me if r == "learner" else snaps[n] if r == "snapshot" else None if r == "none" else r
                   for n, r in enumerate(names)]
    res = simulate("level0", controllers, n_runs=args.eval_runs, n_drones=len(names), racemode=RaceMode.COMPETE,
                   precision=args.precision, seed=args.seed + 1, return_results=True)
    winner, finished = res.winner, res.finish_step >= 0
    print(f"simulate(): {args.eval_runs} races, mean episode time {float(res.episode_times.mean()):.2f} s")
    print(f"{'drone':>5} {'role':>10} {'wins':>6} {'win rate':>9} {'finish rate':>12} {'mean gates':>11}")
    for n, r in enumerate(names):
        wins = int((winner == n).sum())
        print(f"{n:>5} {r:>10} {wins:>6} {wins / args.eval_runs:>9.3f} {float(finished[:, n].mean()):>12.3f} "
              f"{float(res.gates[:, n].mean()):>11.2f}")
    print(f"{'-':>5} {'nobody':>10} {int((winner < 0).sum()):>6}")
    me.close()


if __name__ == "__main__":
    main()
