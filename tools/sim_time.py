"""Cost of one wave step of the batched race evaluation (gym_pybullet_adrp_amd/sim.py): controllers + env step +
results, at level0, E = 4,096, fp64, for (N = 2, both drones scripted) and (N = 4, scripted / policy mixed).

python tools/sim_time.py [--rounds 7] [--envs 4096] [--out profiles/sim_step.json]

Arm A is the fused path: ControllerBank.predict (the policy launches and one race_controller_kernel launch) and
RaceResults.step (one race_results_kernel launch on the handle's own state image).  Arm B is the same loop from
the pieces that were there before: the torch HardCodedCommander.predict, DevicePolicy.act on a contiguous copy of
each policy drone's rows merged into the command arrays with slice assignments, and get_state()-based accounting
kept on the device with torch ops (no host read in either arm).  Both arms launch the same command and step
kernels.  "step_only" is env.step alone on arm A's last command arrays' setpoints (adrp_step(NULL)), and
"step_kernel" the step kernel's own duration from the events on its dispatch.

The method of tools/episode_probe.py: one process, a round runs each arm in turn (interleaved) from a fresh
env.reset(), INNER = 20 steps per timed window and REPLAYS windows between device events; the figure is the median
over the rounds and the margin arm B's own round-to-round spread.  The scripted drones' splines are planned once,
from env 0's reset observation for every env (planning E N distinct starts on the host takes minutes and is not
part of a step); the step's cost does not depend on the spline's values.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_pybullet_adrp_amd.commands import COMMAND_CODE, TIME_SLOT  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander  # noqa: E402
from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.sim import ControllerBank, RaceResults  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Command  # noqa: E402

INNER, REPLAYS = 20, 10


def random_policy(in_dim, seed, hidden=64):
    rng = np.random.default_rng(seed)
    shapes = [(hidden, in_dim), (hidden,), (hidden, hidden), (hidden,), (4, hidden), (4,)]
    w = {k: (rng.normal(size=s) * (0.3 / np.sqrt(s[-1]))).astype(np.float32) for k, s in zip(ACTOR_KEYS, shapes)}
    return DevicePolicy(w, "tanh", 0, "relative")


class TorchAccounts:
    """the results accounting with torch ops on get_state()'s rows (arm B), all on the device"""

    def __init__(self, env):
        E, N, dev = env.num_envs, env.NUM_DRONES, env.device
        names = env.state_field_names()[1]
        self.gi, self.fi, self.E, self.N = names.index("gate"), names.index("flags"), E, N
        self.open = torch.ones(E, dtype=torch.bool, device=dev)
        self.ret = torch.zeros(E, dtype=torch.float64, device=dev)
        self.len = torch.zeros(E, dtype=torch.int32, device=dev)
        self.gates = torch.zeros((E, N), dtype=torch.int32, device=dev)
        self.finish = torch.full((E, N), -1, dtype=torch.int32, device=dev)
        self.elim = torch.full((E, N), -1, dtype=torch.int32, device=dev)
        self.log = [torch.zeros_like(t) for t in (self.ret, self.len, self.gates, self.finish, self.elim)]
        self.left = torch.zeros((), dtype=torch.int64, device=dev)

    def begin(self):
        self.open.fill_(True)
        self.ret.zero_()
        self.len.zero_()
        self.gates.zero_()
        self.finish.fill_(-1)
        self.elim.fill_(-1)

    def step(self, env, rew, term, trunc):
        _, i = env.get_state()
        gate, flags = i[self.gi].view(self.E, self.N), i[self.fi].view(self.E, self.N)
        o = self.open
        self.ret += torch.where(o, rew.double(), 0.0)
        self.len += o.int()
        o2, n2 = o[:, None], self.len[:, None]
        self.gates = torch.where(o2, gate, self.gates)
        self.finish = torch.where(o2 & ((flags & 2) != 0) & (self.finish < 0), n2, self.finish)
        self.elim = torch.where(o2 & ((flags & 1) != 0) & (self.elim < 0), n2, self.elim)
        done = o & (term | trunc)
        for dst, src in zip(self.log, (self.ret, self.len, self.gates, self.finish, self.elim)):
            dst.copy_(torch.where(done if src.dim() == 1 else done[:, None], src, dst))
        self.open = o & ~done
        self.left = self.open.sum()


def timed(run):
    """microseconds per wave step: REPLAYS windows of INNER steps between device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run()
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPLAYS):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (REPLAYS * INNER)


def measure(E, controllers, rounds):
    N = len(controllers)
    env = MultiRaceAviary("level0", num_drones=N, num_envs=E, seed=0, autoreset=False, commands=True)
    obs, _ = env.reset()
    plan_obs = obs[:1].expand(E, N, obs.shape[2]).contiguous()       # env 0's starts for every env (see above)
    pols = {n: random_policy(obs.shape[2], 40 + n) for n, c in enumerate(controllers) if c == "policy"}
    bank = ControllerBank(env, [pols.get(n, c) for n, c in enumerate(controllers)])
    bank.reset(plan_obs)
    hc = HardCodedCommander(plan_obs)
    res, acc = RaceResults(E, N, E, env.device, env.CTRL_FREQ), TorchAccounts(env)
    scripted = torch.tensor([c == "hardcoded" for c in controllers], device=env.device)
    full = COMMAND_CODE[Command.FULLSTATE]
    clock = {"k": 0}

    def restart():
        env.reset()
        bank.phase.zero_()
        hc._flags.zero_()
        res.begin(0, E)
        acc.begin()
        clock["k"] = 0

    def arm_a():
        o = env._obs
        for _ in range(INNER):
            o, rew, term, trunc, _ = env.step(bank.predict(o, clock["k"] / env.CTRL_FREQ))
            res.step(env, rew, term, trunc)
            clock["k"] += 1

    def arm_b():
        o = env._obs
        for _ in range(INNER):
            t = clock["k"] / env.CTRL_FREQ
            codes, args = hc.predict(t)
            if pols:
                codes = torch.where(scripted, codes, 0)
                args = torch.where(scripted[:, None], args, 0.0)
                for n, pol in pols.items():
                    sp = pol.act(o[:, n].contiguous()).double()
                    codes[:, n] = full
                    args[:, n, 0:3] = sp[:, 0:3]
                    args[:, n, 9] = sp[:, 3]
                    args[:, n, TIME_SLOT] = t
            o, rew, term, trunc, _ = env.step((codes, args))
            acc.step(env, rew, term, trunc)
            clock["k"] += 1

    def step_only():
        for _ in range(INNER):
            env.h.step(None, env._obs, env._rew, env._term, env._trunc, env._tobs)

    arms = {"fused": arm_a, "torch": arm_b, "step_only": step_only}
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():
            restart()
            if k == "step_only":
                arm_a()                       # take off first: the same flight regime
            times[k].append(timed(run))
    restart()
    arm_a()
    try:
        env.h.profile_begin(INNER)
        arm_a()
        kern = env.h.profile_end(INNER) * 1e3
    except Exception as e:      # (the figure is an extra: the arms' times above stand without it)
        print(f"step kernel timing unavailable: {e}", flush=True)
        kern = []
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = float(max(times["torch"]) - min(times["torch"]))
    rec = {"E": E, "N": N, "controllers": list(controllers), "precision": "fp64", "kernel": env.kernel_name,
           "fused_us": med["fused"], "torch_us": med["torch"], "step_only_us": med["step_only"],
           "step_kernel_us": float(np.median(kern)) if len(kern) else None,
           "fused_overhead_us": med["fused"] - med["step_only"], "torch_overhead_us": med["torch"] - med["step_only"],
           "saving_us": med["torch"] - med["fused"], "torch_spread_us": spread,
           "fused_spread_us": float(max(times["fused"]) - min(times["fused"])),
           "claim_holds": bool(med["torch"] - med["fused"] > spread), "rounds_us": times}
    for p in pols.values():
        p.close()
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join("profiles", "sim_step.json"))
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_window": INNER,
              "windows_per_round": REPLAYS, "unit": "microseconds per wave step (controllers + env.step + results), "
              "median over the rounds; spread = max - min over the rounds", "configs": []}
    for controllers in (("hardcoded", "hardcoded"), ("hardcoded", "policy", "hardcoded", "policy")):
        rec = measure(args.envs, controllers, args.rounds)
        result["configs"].append(rec)
        print(json.dumps({k: v for k, v in rec.items() if k != "rounds_us"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
