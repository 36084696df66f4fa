"""Cost of one EpisodeStats.step (one adrp_episode_step launch) beside the eager torch ops it replaces:
the ReturnMeter of tools/learn_hover.py (the running return, the sum and the count of the finished
episodes; eight torch ops per env.step, no lengths, no per-episode log).

python tools/episode_probe.py [--rounds 7] [--out profiles/episode_stats.json]

The method of tools/ppo_probe.py: E = 64 and E = 4,096; every arm runs INNER = 20 accounting steps on
fixed step outputs (the constructed stream of tests/episode_reference.py, so episodes do end), eagerly
and as one HIP graph of the 20 steps; a round runs each arm in turn (interleaved) between device events,
the figure is the median over the rounds and the margin the baseline (torch) arm's own round-to-round
spread.  No env steps: the accounting alone.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_pybullet_adrp_amd.evaluation import EpisodeStats  # noqa: E402
from tools.learn_hover import ReturnMeter  # noqa: E402

INNER, REPLAYS = 20, 50


class FixedEnv:
    """what ReturnMeter wraps: step() hands out the prepared outputs of step t % INNER"""

    def __init__(self, rew, term, trunc):
        self.num_envs, self.device = rew.shape[1], rew.device
        self.outs = [(None, rew[t], term[t], trunc[t], None) for t in range(rew.shape[0])]
        self.t = 0

    def step(self, action):
        out = self.outs[self.t % len(self.outs)]
        self.t += 1
        return out


def stream(E):
    t = np.arange(INNER)[:, None]
    e = np.arange(E)[None, :]
    done = (t + 1) % (2 + e % 7) == 0
    rew = (((31 * t + 17 * e) % 64 - 20) / 8).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (rew, done & (e % 2 == 0), done & (e % 2 == 1)))


def graph_of(fn, side):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            fn()
    return g


def timed(run):
    """microseconds per accounting step: REPLAYS runs of INNER steps between device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run()
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPLAYS):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (REPLAYS * INNER)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "episode_stats.json"))
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_graph": INNER,
              "replays_per_round": REPLAYS, "unit": "microseconds per accounting step, median over the rounds", "sizes": []}
    side = torch.cuda.Stream()
    for E in (64, 4096):
        rew, term, trunc = stream(E)
        st = EpisodeStats(E, 0, capacity=100, ring=True)
        meter = ReturnMeter(FixedEnv(rew, term, trunc))

        def kernel():
            for t in range(INNER):
                st.step(rew[t], term[t], trunc[t])

        def torch_ops():
            for _ in range(INNER):
                meter.step(None)
        arms = {"kernel_eager": kernel, "torch_eager": torch_ops}
        arms["kernel_graph"] = graph_of(kernel, side).replay
        arms["torch_graph"] = graph_of(torch_ops, side).replay
        times = {k: [] for k in arms}
        with torch.cuda.stream(side):
            for _ in range(args.rounds):
                for k, run in arms.items():
                    times[k].append(timed(run))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(max(times[k]) - min(times[k])) for k in ("torch_eager", "torch_graph")}
        rec = {"E": E, **{f"{k}_us": v for k, v in med.items()},
               "torch_eager_spread_us": spread["torch_eager"], "torch_graph_spread_us": spread["torch_graph"],
               "eager_saving_us": med["torch_eager"] - med["kernel_eager"], "graph_saving_us": med["torch_graph"] - med["kernel_graph"],
               "rounds_us": times}
        result["sizes"].append(rec)
        print(json.dumps({k: v for k, v in rec.items() if k != "rounds_us"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
