"""Per-drone PPO on a multi-drone race: tools/learn_hover.py's loop on MultiRaceAviary(COMPETE, autoreset=False).

python tools/learn_race.py [--envs 256] [--drones 4] [--n-steps 128] [--iterations 20] [--batch-size 1024]
                           [--n-epochs 10] [--seed 0] [--precision fp32] [--out FILE] [--save policy.pth]

Every drone is an agent of one shared policy (49 inputs: the drone's own state, the gates, the obstacles and the
gate id; four outputs, RLController's relative FULLSTATE setpoint); the reward is the RewardWrapper's, per drone.
Per iteration: MultiAgentRolloutCollector.collect() (n_steps env.steps of every env), PPOLearner.train() on the
valid samples (a drone that was eliminated or finished gives none until its env is reset), then one line with
episode_summary(): the mean return and length of the agent episodes that ended during the rollout (raw rewards,
without the time-limit bootstrap).  The reference cannot run this loop: its README lists training more than one
agent in MultiRaceAviary as a limitation of its sub-process controllers.  No learning bar is set here.
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
from gym_pybullet_adrp_amd.ppo import PPOLearner  # noqa: E402
from gym_pybullet_adrp_amd.rollout import MultiAgentRolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import RaceMode  # noqa: E402
from tools.learn_hover import sb3_init  # noqa: E402


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
    args = ap.parse_args()
    env = MultiRaceAviary("level0", num_drones=args.drones, racemode=RaceMode.COMPETE, num_envs=args.envs, seed=args.seed,
                          precision=args.precision, autoreset=False)
    pol = DevicePolicy(sb3_init(49, 64, 4, args.seed), "tanh", 0, "relative")
    col = MultiAgentRolloutCollector(env, pol, args.n_steps, seed=args.seed)
    learner = PPOLearner(pol, n_epochs=args.n_epochs, batch_size=args.batch_size, seed=args.seed)
    col.reset()
    log, samples, t0 = [], 0, time.time()
    for it in range(args.iterations):
        col.collect()
        stats = learner.train(col)
        valid = int(col.valid.sum())
        samples += valid
        s = stats[-1].mean(0).cpu().tolist()
        rec = {"iteration": it, "valid_samples": samples, "valid_fraction": valid / (col.T * col.E),
               "policy_loss": s[0], "value_loss": s[1], "approx_kl": s[3], "clip_fraction": s[4],
               "wall_s": round(time.time() - t0, 3)}
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
    learner.close()
    pol.close()
    env.close()


if __name__ == "__main__":
    main()
