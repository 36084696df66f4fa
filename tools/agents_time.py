"""Cost of the per-drone agents' bookkeeping in a MultiAgentRolloutCollector step, by device events.

python tools/agents_time.py [--envs 4096] [--drones 4] [--steps 60] [--rounds 7] [--level level3] [--out profiles/race_agents.json]

Three arms walk the collector's step sequence on the same env, policy and buffers (fp64, COMPETE), interleaved
round by round, each from a fresh reset after warm-up steps of its own:
  step   the sequence without the agents' bookkeeping: sample launch, env.step, critic values of the post-step
         rows, masked env.reset, the row copies (the rewards are not written)
  fused  the collector's own step: the same plus one adrp_race_agents_step_env launch and one
         adrp_race_agents_reset launch
  torch  the same bookkeeping from the pieces that were there before: get_state()'s gate / flags rows and eager
         torch ops on [E N] tensors (the RewardWrapper per drone in float64, validity, bootstrap, starts, episode
         sums, the masked re-initialisation)
Reported per arm: microseconds per collector step, the median and the min / max over the rounds; the fused
arm's overhead over "step", and its saving against "torch" beside that arm's round-to-round spread.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.policy import DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.rollout import MultiAgentRolloutCollector  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Physics, RaceMode  # noqa: E402
from tools.learn_hover import sb3_init  # noqa: E402


class TorchAgents:
    """the agents kernels' bookkeeping as eager torch ops (the arm the fused launch is measured against)"""

    def __init__(self, col):
        self.col, env = col, col.env
        R, dev = col.E, env.device
        self.N, self.G = col.N, int(env.cfg.track.num_gates)
        names = env.state_field_names()[1]
        self.gi, self.fi = names.index("gate"), names.index("flags")
        self.wr_gate = torch.zeros(R, dtype=torch.int32, device=dev)
        self.target, self.prev = torch.zeros((R, 3), dtype=torch.float64, device=dev), torch.zeros((R, 3), dtype=torch.float64, device=dev)
        self.alive = torch.zeros(R, dtype=torch.bool, device=dev)
        self.run_return = torch.zeros(R, dtype=torch.float64, device=dev)
        self.run_length = torch.zeros(R, dtype=torch.int32, device=dev)

    def reset(self, obs, mask=None):
        rows = obs.view(self.col.E, -1)
        m = torch.ones(self.col.E, dtype=torch.bool, device=rows.device) if mask is None else mask.bool().repeat_interleave(self.N)
        self.wr_gate = torch.where(m, rows[:, 48].to(torch.int32), self.wr_gate)
        self.target = torch.where(m[:, None], rows[:, 12:15].double(), self.target)
        self.prev = torch.where(m[:, None], rows[:, 0:3].double(), self.prev)
        self.alive = self.alive | m
        self.run_return = torch.where(m, 0.0, self.run_return)
        self.run_length = torch.where(m, 0, self.run_length)

    def step(self, t, obs, term, trunc, tv):
        col, R = self.col, self.col.E
        _, i = col.env.get_state()
        gate, flags = i[self.gi], i[self.fi]
        row = obs.view(R, -1).double()
        was, done, fin = self.alive, (flags & 3) != 0, (flags & 2) != 0
        newly = was & done
        te, tr = term.repeat_interleave(self.N), trunc.repeat_interleave(self.N)
        passed = gate > torch.fmod(self.wr_gate, 4)
        move = passed & (gate >= 0) & (gate < 4) & (gate < self.G)
        gates = row[:, 12:28].view(R, 4, 4)[:, :, :3]
        pick = gates.gather(1, gate.clamp(0, 3).long().view(R, 1, 1).expand(R, 1, 3)).squeeze(1)
        tgt = torch.where(move[:, None], pick, self.target)
        pos = row[:, 0:3]
        pxy, cxy = (tgt[:, :2] - self.prev[:, :2]).norm(dim=1), (tgt[:, :2] - pos[:, :2]).norm(dim=1)
        pz, cz = (tgt[:, 2] - self.prev[:, 2]).abs(), (tgt[:, 2] - pos[:, 2]).abs()
        r = (pxy - cxy) + (pz - cz) + torch.where(passed, 5.0, 0.0) + torch.where(newly & ~fin, -1.0, 0.0) \
            + torch.where(newly & fin, 10.0, 0.0)
        boot = was & ~done & tr & ~te
        stored = torch.where(boot, r + col.gamma * tv.double(), r)
        col.rewards[t] = torch.where(was, stored.float(), 0.0)
        col.valid[t] = was.to(torch.uint8)
        col._last_start.copy_((done | te | tr).float())
        ends = newly | (was & (te | tr))
        ret, length = self.run_return + r, self.run_length + 1
        col.ep_return[t] = torch.where(ends, ret, float("nan"))
        col.ep_length[t] = torch.where(ends, length, 0)
        self.wr_gate = torch.where(was & passed, gate, self.wr_gate)
        self.target = torch.where(was[:, None], tgt, self.target)
        self.prev = torch.where(was[:, None], pos, self.prev)
        self.run_return = torch.where(was, ret, self.run_return)
        self.run_length = torch.where(was, length, self.run_length)
        self.alive = was & ~done


def run_arm(col, arm, steps, torch_agents):
    """`steps` collector steps of one arm (buffer row t % T)"""
    env, R = col.env, col.E
    env_act = col._env_act.view(R, 4)
    for k in range(steps):
        t = k % col.T
        col.obs[t].copy_(col._last_obs)
        col._sample_row(t, k, env_act)
        obs, _, term, trunc, _ = env.step(col._env_act)
        col._values_of(obs.view(R, -1), col._tv)
        if arm == "fused":
            col._check(col.lib.adrp_race_agents_step_env(
                col._ref, env.h.h, obs.data_ptr(), term.data_ptr(), trunc.data_ptr(), col._tv.data_ptr(), col.gamma,
                col.rewards[t].data_ptr(), col.valid[t].data_ptr(), col._last_start.data_ptr(), col.ep_return[t].data_ptr(),
                col.ep_length[t].data_ptr(), col._stream()), "adrp_race_agents_step_env")
        elif arm == "torch":
            torch_agents.step(t, obs, term, trunc, col._tv)
        torch.bitwise_or(term, trunc, out=col._mask)
        mask = col._mask.view(torch.uint8)
        obs, _ = env.reset(mask=mask)
        if arm == "fused":
            col._agents_reset(obs, mask)
        elif arm == "torch":
            torch_agents.reset(obs, mask)
        col._last_obs.copy_(obs.view(R, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--drones", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--level", default="level3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agents_time.py measures on the GPU: no HIP device is visible")
    env = MultiRaceAviary(args.level, num_drones=args.drones, physics=Physics.PYB_DW, racemode=RaceMode.COMPETE,
                          num_envs=args.envs, seed=1, precision="fp64", autoreset=False)
    pol = DevicePolicy(sb3_init(49, 64, 4, 0), "tanh", 0, "relative")
    col = MultiAgentRolloutCollector(env, pol, min(args.steps, 64), seed=0)
    ta = TorchAgents(col)
    arms = ("step", "fused", "torch")
    times = {a: [] for a in arms}
    checks = {}
    with torch.cuda.device(env.device):
        for r in range(args.rounds):
            for a in arms[r % 3:] + arms[:r % 3]:          # rotate the order round by round
                env.h.reseed(1)                             # every arm flies the same episodes
                col.reset()
                ta.reset(env._obs)
                run_arm(col, a, args.warmup, ta)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                run_arm(col, a, args.steps, ta)
                stop.record()
                stop.synchronize()
                times[a].append(start.elapsed_time(stop) * 1e3 / args.steps)
                if r == 0 and a != "step":                  # the two arms account the same rollout: equal sums
                    checks[a] = (float(col.rewards.double().sum()), int(col.valid.sum()), int(col.ep_length.sum()))
    med = {a: statistics.median(v) for a, v in times.items()}
    out = {"envs": args.envs, "drones": args.drones, "precision": "fp64", "level": args.level, "kernel": env.kernel_name,
           "steps_per_round": args.steps, "rounds": args.rounds,
           "us_per_step": {a: {"median": med[a], "min": min(v), "max": max(v), "rounds": v} for a, v in times.items()},
           "fused_overhead_over_step_us": med["fused"] - med["step"],
           "torch_overhead_over_step_us": med["torch"] - med["step"],
           "fused_saving_against_torch_us": med["torch"] - med["fused"],
           "torch_round_to_round_spread_us": max(times["torch"]) - min(times["torch"]),
           "first_round_sums (rewards, valid, ep_length)": checks}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    pol.close()
    env.close()


if __name__ == "__main__":
    main()
