"""examples/learn.py's loop on the device: PPO on HoverAviary(act=ONE_D_RPM).

python tools/learn_hover.py [--envs 64] [--n-steps 256] [--iterations 60] [--batch-size 256] [--seed 0] [--out FILE]
                            [--eval-freq N] [--eval-episodes 5] [--eval-envs 1] [--target-reward R] [--best FILE]

Per iteration: RolloutCollector.collect() (n_steps env.steps of every env), PPOLearner.train()
(n_epochs passes of minibatch updates), then one line with the mean return of the episodes that
ended during the rollout (the env's own rewards, summed per episode; the time-limit bootstrap the
collector adds to the stored rewards is not in it).  SB3's MlpPolicy initialisation: orthogonal
weights (gain sqrt 2 on the hidden layers, 0.01 on action_net, 1 on value_net), zero biases,
log_std 0.  The reference's stopping threshold is 474.15 (learn.py:79) of the 480 a perfect
8 s episode at 30 Hz collects; no bar is set here.

Every line also carries ep_rew_mean / ep_len_mean, SB3's Monitor window: the last 100 episodes of an
EpisodeStats ring attached to the collector.  --eval-freq N adds learn.py:58-91's evaluation: a second
HoverAviary (--eval-envs envs) and an Evaluator that runs --eval-episodes deterministic episodes at the
first rollout boundary after every N env.step calls, keeps the best parameters in --best, and stops the
run once the best evaluation mean reaches --target-reward (eval_mean on the iterations that evaluated).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_pybullet_adrp_amd.envs.hover import HoverAviary  # noqa: E402
from gym_pybullet_adrp_amd.evaluation import EpisodeStats, Evaluator  # noqa: E402
from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, CRITIC_KEYS, DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.ppo import PPOLearner  # noqa: E402
from gym_pybullet_adrp_amd.rollout import RolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import ActionType  # noqa: E402


def sb3_init(in_dim, hidden, act_dim, seed):
    g = torch.Generator().manual_seed(seed)

    def ortho(o, i, gain):
        w = torch.empty(o, i)
        torch.nn.init.orthogonal_(w, gain=gain, generator=g)
        return w.numpy(), torch.zeros(o).numpy()
    wd = dict(zip(ACTOR_KEYS, ortho(hidden, in_dim, math.sqrt(2)) + ortho(hidden, hidden, math.sqrt(2)) + ortho(act_dim, hidden, 0.01)))
    wd.update(zip(CRITIC_KEYS, ortho(hidden, in_dim, math.sqrt(2)) + ortho(hidden, hidden, math.sqrt(2)) + ortho(1, hidden, 1.0)
                  + (torch.zeros(act_dim).numpy(),)))
    return wd


class ReturnMeter:
    """sums the env's rewards per episode on the device (wraps env.step; nothing is read back per step)"""

    def __init__(self, env):
        self.env, self._step = env, env.step
        E, dev = env.num_envs, env.device
        self.run = torch.zeros(E, device=dev)
        self.total = torch.zeros((), device=dev)
        self.count = torch.zeros((), device=dev)
        env.step = self.step

    def step(self, action):
        out = self._step(action)
        done = (out[2] | out[3]).to(torch.float32)
        self.run += out[1]
        self.total += (self.run * done).sum()
        self.count += done.sum()
        self.run *= 1.0 - done
        return out

    def read(self):
        total, count = float(self.total), float(self.count)
        self.total.zero_()
        self.count.zero_()
        return (total / count if count else float("nan")), int(count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--n-steps", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--eval-freq", type=int, default=0, help="evaluate every N env.step calls (0: never)")
    ap.add_argument("--eval-episodes", type=int, default=5)
    ap.add_argument("--eval-envs", type=int, default=1)
    ap.add_argument("--target-reward", type=float, default=None)
    ap.add_argument("--best", default=None, help="policy.pth-style file of the best evaluated parameters")
    args = ap.parse_args()
    env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=args.envs, seed=args.seed)
    meter = ReturnMeter(env)
    pol = DevicePolicy(sb3_init(env.h.D, 64, 1, args.seed), "tanh", 0, "raw")
    window = EpisodeStats(args.envs, env.device, capacity=100, ring=True)
    col = RolloutCollector(env, pol, args.n_steps, seed=args.seed, episode_stats=window)
    learner = PPOLearner(pol, n_epochs=args.n_epochs, batch_size=args.batch_size, seed=args.seed)
    evaluator = eval_env = None
    if args.eval_freq > 0:
        eval_env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=args.eval_envs, seed=args.seed)
        evaluator = Evaluator(eval_env, pol, n_eval_episodes=args.eval_episodes, eval_freq=args.eval_freq,
                              reward_threshold=args.target_reward, best_path=args.best)
    col.reset()
    log, samples, t0 = [], 0, time.time()
    for it in range(args.iterations):
        col.collect()
        stats = learner.train(col)
        samples += args.n_steps * args.envs
        ret, episodes = meter.read()
        s = stats[-1].mean(0).cpu().tolist()
        rec = {"iteration": it, "samples": samples, "episodes": episodes, "mean_episode_return": ret,
               "policy_loss": s[0], "value_loss": s[1], "approx_kl": s[3], "clip_fraction": s[4],
               "wall_s": round(time.time() - t0, 3)}
        w = window.summary()
        rec["ep_rew_mean"], rec["ep_len_mean"] = w["ep_rew_mean"], w["ep_len_mean"]
        go_on = True
        if evaluator is not None:
            go_on = evaluator.on_rollout(samples, (it + 1) * args.n_steps, learner)
            if evaluator.evaluated:
                rec["eval_mean"], rec["eval_len_mean"] = evaluator.last_mean_reward, evaluator.last_mean_length
        log.append(rec)
        print(json.dumps(rec), flush=True)
        if not go_on:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"args": vars(args), "log": log}, f, indent=1)
            f.write("\n")
    learner.close()
    pol.close()
    env.close()
    if eval_env is not None:
        eval_env.close()


if __name__ == "__main__":
    main()
