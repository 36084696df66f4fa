"""Cost of a RosterRolloutCollector step, by device events, with tools/agents_time.py's method.

python tools/roster_time.py [--envs 4096] [--drones 4] [--steps 60] [--rounds 7] [--level level0] [--out profiles/race_roster.json]

Five arms (fp64, COMPETE), interleaved round by round in rotated order, each a rollout of --steps collector steps
(GAE included) from a fresh reset of the same seed after a warm-up rollout of its own:
  learners    (a) RosterRolloutCollector, every drone a learner (command-mode env)
  opponents   (b) RosterRolloutCollector, one learner against scripted HardCodedController drones
  opponents_learners  (b) with end_on="learners": an env is reset with its last learner, not with its race
  setpoint    (c) MultiAgentRolloutCollector on the setpoint-mode env: the nearest equivalent of (a) that was there
              before the roster collector
  pieces      (d) the work of (b) from the pieces that were there before it, on (b)'s env and buffers: the scripted
              drones through HardCodedCommander.predict on a torch [E] clock tensor (ControllerBank's launch takes
              one scalar clock for all envs, so it cannot follow per-env resets), the learner's command row, the
              clocks and the flag clearing as eager torch ops, the full-width adrp_race_agents_step_env and a gather
              of the learner's columns
Reported per arm: microseconds per collector step, the median and the min / max over the rounds; (b) - (d) beside
(d)'s round-to-round spread, and (a) - (c); for the two (b) arms the valid rows of the timed rollout and valid rows per
second.  The scripted drones plan on the device (one launch per reset).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_pybullet_adrp_amd.commands import COMMAND_CODE, TIME_SLOT  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.rollout import MultiAgentRolloutCollector, RosterRolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Command, RaceMode  # noqa: E402
from tools.learn_hover import sb3_init  # noqa: E402


class Pieces:
    """arm (d): one learner (drone 0) against scripted drones, on a RosterRolloutCollector's env, commander, agent
    state and buffers, without the roster launches"""

    def __init__(self, col):
        self.col = col
        E, N, dev = col.num_envs, col.N, col.env.device
        self.clock = torch.zeros(E, dtype=torch.float64, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.boot = torch.zeros(E * N, **f32)
        self.rewards, self.next_start = torch.zeros(E * N, **f32), torch.zeros(E * N, **f32)
        self.valid = torch.zeros(E * N, dtype=torch.uint8, device=dev)
        self.ep_return = torch.zeros(E * N, dtype=torch.float64, device=dev)
        self.ep_length = torch.zeros(E * N, dtype=torch.int32, device=dev)
        self.fullstate = COMMAND_CODE[Command.FULLSTATE]

    def reset(self):
        col = self.col
        col.reset()                                   # env.reset, the plan, the agents' reset (and the roster's clocks)
        col.commander._flags.zero_()
        self.clock.zero_()

    def collect(self):
        col = self.col
        env, E, N, cm = col.env, col.num_envs, col.N, col.commander
        obs, base = col._env_obs, col.rollouts * col.T
        env_act = col.learner_act.view(E, 4)
        for t in range(col.T):
            col.obs[t].copy_(obs[:, 0])
            col._sample_row(t, base + t, env_act)
            ep_time = self.clock / float(env.CTRL_FREQ)
            codes, args = cm.predict(ep_time)
            codes[:, 0] = self.fullstate
            args[:, 0] = 0.0
            args[:, 0, 0:3] = env_act[:, 0:3]
            args[:, 0, 9] = env_act[:, 3]
            args[:, 0, TIME_SLOT] = ep_time
            obs, _, term, trunc, _ = env.step((codes, args))
            col._post.copy_(obs[:, 0])
            col._values_of(col._post, col._tv)
            self.boot.view(E, N)[:, 0] = col._tv
            col._check(col.lib.adrp_race_agents_step_env(
                col._ref, env.h.h, obs.data_ptr(), term.data_ptr(), trunc.data_ptr(), self.boot.data_ptr(), col.gamma,
                self.rewards.data_ptr(), self.valid.data_ptr(), self.next_start.data_ptr(), self.ep_return.data_ptr(),
                self.ep_length.data_ptr(), col._stream()), "adrp_race_agents_step_env")
            col.rewards[t].copy_(self.rewards.view(E, N)[:, 0])
            col.valid[t].copy_(self.valid.view(E, N)[:, 0])
            col._last_start.copy_(self.next_start.view(E, N)[:, 0])
            col.ep_return[t].copy_(self.ep_return.view(E, N)[:, 0])
            col.ep_length[t].copy_(self.ep_length.view(E, N)[:, 0])
            torch.bitwise_or(term, trunc, out=col._mask)
            mask = col._mask.view(torch.uint8)
            obs, _ = env.reset(mask=mask)
            col._agents_reset(obs, mask)
            self.clock = torch.where(col._mask, 0.0, self.clock + 1.0)
            cm._flags &= ~col._mask[None, :, None]
        col._env_obs = obs
        col._post.copy_(obs[:, 0])
        col._finish(col._post)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--drones", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--level", default="level0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roster_time.py measures on the GPU: no HIP device is visible")
    N = args.drones

    def make_env(commands):
        return MultiRaceAviary(args.level, num_drones=N, racemode=RaceMode.COMPETE, num_envs=args.envs, seed=1, precision="fp64",
                               autoreset=False, commands=commands)

    pol = DevicePolicy(sb3_init(49, 64, 4, 0), "tanh", 0, "relative")
    env_a, env_b, env_c, env_e = make_env(True), make_env(True), make_env(False), make_env(True)
    col_a = RosterRolloutCollector(env_a, pol, ["learner"] * N, args.steps, seed=0)
    col_b = RosterRolloutCollector(env_b, pol, ["learner"] + ["hardcoded"] * (N - 1), args.steps, seed=0, planner="device")
    col_c = MultiAgentRolloutCollector(env_c, pol, args.steps, seed=0)
    col_e = RosterRolloutCollector(env_e, pol, ["learner"] + ["hardcoded"] * (N - 1), args.steps, seed=0, planner="device",
                                   end_on="learners")
    pieces = Pieces(col_b)
    arms = {"learners": (col_a, col_a), "opponents": (col_b, col_b), "setpoint": (col_c, col_c), "pieces": (pieces, col_b),
            "opponents_learners": (col_e, col_e)}
    order = tuple(arms)
    times = {a: [] for a in arms}
    checks = {}
    with torch.cuda.device(env_a.device):
        for r in range(args.rounds):
            for a in order[r % len(order):] + order[:r % len(order)]:          # rotate the order round by round
                runner, col = arms[a]
                col.env.h.reseed(1)                            # every round flies the same episodes
                col.rollouts = 0
                runner.reset()
                runner.collect()                               # warm-up
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                runner.collect()
                stop.record()
                stop.synchronize()
                times[a].append(start.elapsed_time(stop) * 1e3 / args.steps)
                if r == 0:                                     # (b) and (d) account the same rollout: equal sums
                    checks[a] = (float(col.rewards.double().sum()), int(col.valid.sum()), int(col.ep_length.sum()))
    med = {a: statistics.median(v) for a, v in times.items()}
    # every round flies the same episodes, so the first round's valid rows are every round's
    rows = {a: {"valid_rows_per_rollout": checks[a][1], "rows_per_rollout": arms[a][1].T * arms[a][1].E,
                "valid_rows_per_second": checks[a][1] / (med[a] * 1e-6 * args.steps)} for a in ("opponents", "opponents_learners")}
    out = {"envs": args.envs, "drones": N, "precision": "fp64", "level": args.level, "kernel_command_mode": env_b.kernel_name,
           "kernel_setpoint_mode": env_c.kernel_name, "steps_per_round": args.steps, "rounds": args.rounds,
           "us_per_step": {a: {"median": med[a], "min": min(v), "max": max(v), "rounds": v} for a, v in times.items()},
           "opponents_minus_pieces_us": med["opponents"] - med["pieces"],
           "pieces_round_to_round_spread_us": max(times["pieces"]) - min(times["pieces"]),
           "learners_minus_setpoint_us": med["learners"] - med["setpoint"],
           "setpoint_round_to_round_spread_us": max(times["setpoint"]) - min(times["setpoint"]),
           "end_on": rows,
           "valid_rows_per_second_learners_over_env": rows["opponents_learners"]["valid_rows_per_second"] /
           rows["opponents"]["valid_rows_per_second"],
           "first_round_sums (rewards, valid, ep_length)": checks}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    pol.close()
    for e in (env_a, env_b, env_c, env_e):
        e.close()


if __name__ == "__main__":
    main()
