"""examples/learn.py's loop on the device: PPO on HoverAviary(act=ONE_D_RPM).

python tools/learn_hover.py [--envs 64] [--n-steps 256] [--iterations 60] [--batch-size 256] [--seed 0] [--out FILE]
                            [--eval-freq N] [--eval-episodes 5] [--eval-envs 1] [--target-reward R] [--best FILE]
                            [--target-kl K] [--learning-rate 3e-4] [--clip-range 0.2] [--lr-schedule constant|linear]
                            [--clip-schedule constant|linear]

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

--target-kl is SB3's early stop of a train() (a latch on the device; every line then carries stop_info(): whether
and at which epoch / minibatch it stopped, and the optimizer steps applied).  The linear schedules go from the
given value towards 0 over the run, evaluated at progress_remaining = 1 - num_timesteps / total_timesteps with the
timesteps collected before the rollout being trained on, so the last rollout still trains at 1 / iterations of the
start value (SB3 counts the rollout just collected and ends at a rate of 0, which adrp_ppo_set_rates refuses).
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
from gym_pybullet_adrp_amd.ppo import PPOLearner, linear_schedule  # noqa: E402
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


def rates(args):
    """PPOLearner's learning_rate / clip_range from --learning-rate, --clip-range and the two schedule switches"""
    return {"learning_rate": linear_schedule(args.learning_rate) if args.lr_schedule == "linear" else args.learning_rate,
            "clip_range": linear_schedule(args.clip_range) if args.clip_schedule == "linear" else args.clip_range}


def last_epoch_stats(learner, stats):
    """the mean statistics of the last epoch that ran (with a target_kl: of its minibatches up to the one that tripped
    the stop, found through the one host read stop_info()) -> ([5], stop_info() or None)"""
    if learner.target_kl is None:
        return stats[-1].mean(0).cpu().tolist(), None
    stop = learner.stop_info()
    return torch.nanmean(stats[stop["epoch"] if stop["stopped"] else -1], 0).cpu().tolist(), stop


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
    ap.add_argument("--target-kl", type=float, default=None, help="SB3's target_kl: stop a train() once approx_kl > 1.5 x this")
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--clip-range", type=float, default=0.2)
    ap.add_argument("--lr-schedule", default="constant", choices=("constant", "linear"), help="linear: to 0 at the end of the run")
    ap.add_argument("--clip-schedule", default="constant", choices=("constant", "linear"))
    args = ap.parse_args()
    env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=args.envs, seed=args.seed)
    meter = ReturnMeter(env)
    pol = DevicePolicy(sb3_init(env.h.D, 64, 1, args.seed), "tanh", 0, "raw")
    window = EpisodeStats(args.envs, env.device, capacity=100, ring=True)
    col = RolloutCollector(env, pol, args.n_steps, seed=args.seed, episode_stats=window)
    learner = PPOLearner(pol, n_epochs=args.n_epochs, batch_size=args.batch_size, seed=args.seed, **rates(args))
    learner.set_target_kl(args.target_kl)
    evaluator = eval_env = None
    if args.eval_freq > 0:
        eval_env = HoverAviary(act=ActionType.ONE_D_RPM, num_envs=args.eval_envs, seed=args.seed)
        evaluator = Evaluator(eval_env, pol, n_eval_episodes=args.eval_episodes, eval_freq=args.eval_freq,
                              reward_threshold=args.target_reward, best_path=args.best)
    col.reset()
    log, samples, t0 = [], 0, time.time()
    for it in range(args.iterations):
        col.collect()
        samples += args.n_steps * args.envs
        stats = learner.train(col, progress_remaining=1.0 - it / args.iterations)
        ret, episodes = meter.read()
        s, stop = last_epoch_stats(learner, stats)
        rec = {"iteration": it, "samples": samples, "episodes": episodes, "mean_episode_return": ret,
               "policy_loss": s[0], "value_loss": s[1], "approx_kl": s[3], "clip_fraction": s[4],
               "wall_s": round(time.time() - t0, 3)}
        if stop is not None:
            rec["stop_info"] = stop
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
