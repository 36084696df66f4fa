"""Time of one PPO minibatch update: the fused on-device update (PPOLearner.update, four launches)
beside torch doing the same update in float32 on the GPU (gather the minibatch, forward, the loss of
SB3 2.3.2 PPO.train(), backward, clip_grad_norm_, Adam(eps=1e-5)), eager and graph-captured.

python tools/ppo_probe.py [--rounds 7] [--out profiles/ppo_update.json] [--errors FILE]
python tools/ppo_probe.py launches N      200 fused updates of N rows (a rocprofv3 --kernel-trace --stats target)

The method of tools/policy_probe.py wide: every graph arm is one HIP graph of INNER updates, a round
replays each arm in turn (interleaved) between device events, the figure is the median over the
rounds and the margin the torch graph arm's own round-to-round spread.  The eager torch arm runs the
same INNER updates un-captured between the same events.  Shapes 72-64-64-4 and 144-64-64-8, minibatch
n = 64, 4096 and 65536 rows out of a 2 n-row buffer.  Also one full train() (10 epochs) beside the
collect() that feeds it: HoverAviary(RPM), 4096 envs x 128 steps, batch_size 4096.  --errors: the
JSON lines tests/test_ppo_update_gpu.py writes under ADRP_PPO_ERRORS, copied into the output.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, CRITIC_KEYS, DevicePolicy  # noqa: E402
from gym_pybullet_adrp_amd.ppo import PPOLearner  # noqa: E402

KEYS = ACTOR_KEYS + CRITIC_KEYS
INNER, REPLAYS = 20, 5


def random_net(rng, in_dim, h, out):
    def lin(o, i, gain):
        return ((rng.standard_normal((o, i)) * gain / math.sqrt(i)).astype(np.float32), np.zeros(o, np.float32))
    wd = dict(zip(ACTOR_KEYS, lin(h, in_dim, math.sqrt(2)) + lin(h, h, math.sqrt(2)) + lin(out, h, 0.01)))
    wd.update(zip(CRITIC_KEYS, lin(h, in_dim, math.sqrt(2)) + lin(h, h, math.sqrt(2)) + lin(1, h, 1.0) + (np.zeros(out, np.float32),)))
    return wd


class TorchPPO:
    """the same update in torch float32 on the device (capturable Adam, so that it can be graphed)"""

    def __init__(self, wd, bufs, idx, clip=0.2, vf_coef=0.5, max_grad_norm=0.5):
        self.p = {k: torch.from_numpy(wd[k]).cuda().requires_grad_(True) for k in KEYS}
        self.params = [self.p[k] for k in KEYS]
        self.opt = torch.optim.Adam(self.params, lr=3e-4, eps=1e-5, capturable=True)
        self.bufs, self.idx, self.clip, self.vf_coef, self.max_grad_norm = bufs, idx, clip, vf_coef, max_grad_norm

    def mlp(self, x, pre, head):
        p = self.p
        h = torch.tanh(torch.nn.functional.linear(x, p[f"mlp_extractor.{pre}.0.weight"], p[f"mlp_extractor.{pre}.0.bias"]))
        h = torch.tanh(torch.nn.functional.linear(h, p[f"mlp_extractor.{pre}.2.weight"], p[f"mlp_extractor.{pre}.2.bias"]))
        return torch.nn.functional.linear(h, p[f"{head}.weight"], p[f"{head}.bias"])

    def update(self):
        obs, actions, old_values, old_lp, adv, ret = (b.index_select(0, self.idx) for b in self.bufs)
        mean, values = self.mlp(obs, "policy_net", "action_net"), self.mlp(obs, "value_net", "value_net")[:, 0]
        ls = self.p["log_std"]
        lp = (-((actions - mean) ** 2) / (2 * torch.exp(ls) ** 2) - ls - math.log(math.sqrt(2 * math.pi))).sum(1)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(lp - old_lp)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - self.clip, 1 + self.clip)).mean()
        value_loss = torch.nn.functional.mse_loss(ret, values)
        loss = policy_loss + self.vf_coef * value_loss          # ent_coef 0
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
        self.opt.step()


def graph_of(fn, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(INNER):
                fn()
    return g


def timed(run):
    """microseconds per update: REPLAYS runs of INNER updates between device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run()
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPLAYS):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (REPLAYS * INNER)


def updates(args, result):
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()
    for in_dim, h, out in ((72, 64, 4), (144, 64, 8)):
        for n in (64, 4096, 65536):
            wd = random_net(rng, in_dim, h, out)
            rows = 2 * n
            bufs = (torch.randn((rows, in_dim), device="cuda"), torch.randn((rows, out), device="cuda") * 0.5,
                    torch.randn(rows, device="cuda"), torch.randn(rows, device="cuda") * 0.3 - 0.92 * out,
                    torch.randn(rows, device="cuda"), torch.randn(rows, device="cuda"))
            idx = torch.randperm(rows, device="cuda")[:n].contiguous()
            pol = DevicePolicy(wd, "tanh", 0, "raw")
            learner = PPOLearner(pol)
            stats = torch.zeros(5, device="cuda")
            ref = TorchPPO(wd, bufs, idx)

            def fused():
                learner.update(*bufs, idx, stats=stats)

            def eager():
                for _ in range(INNER):
                    ref.update()
            with torch.cuda.stream(stream):
                eager()
            g_fused, g_torch = graph_of(fused, stream), graph_of(ref.update, stream)
            arms = {"fused_graph": g_fused.replay, "torch_graph": g_torch.replay, "torch_eager": eager}
            times = {k: [] for k in arms}
            with torch.cuda.stream(stream):
                for _ in range(args.rounds):
                    for k, run in arms.items():
                        times[k].append(timed(run))
            med = {k: float(np.median(v)) for k, v in times.items()}
            spread = float(max(times["torch_graph"]) - min(times["torch_graph"]))
            rec = {"shape": f"{in_dim}-{h}-{h}-{out}", "n": n, "fused_us": med["fused_graph"], "torch_graph_us": med["torch_graph"],
                   "torch_eager_us": med["torch_eager"], "torch_graph_spread_us": spread, "rounds_us": times,
                   "fused_beats_torch_graph": med["fused_graph"] < med["torch_graph"] - spread}
            result["updates"].append(rec)
            print(json.dumps({k: v for k, v in rec.items() if k != "rounds_us"}), flush=True)
            learner.close()
            pol.close()


def train_vs_collect(result, envs=4096, n_steps=128, batch_size=4096, n_epochs=10):
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.rollout import RolloutCollector
    env = HoverAviary(num_envs=envs, seed=1, initial_xyzs=[0, 0, 1.0])
    pol = DevicePolicy(random_net(np.random.default_rng(1), 72, 64, 4), "tanh", 0, "raw")
    col = RolloutCollector(env, pol, n_steps, seed=1)
    learner = PPOLearner(pol, n_epochs=n_epochs, batch_size=batch_size)
    col.reset()
    col.collect()
    learner.train(col)
    t = {"collect_ms": [], "train_ms": []}
    for _ in range(3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        col.collect()
        ev[1].record()
        learner.train(col)
        ev[2].record()
        torch.cuda.synchronize()
        t["collect_ms"].append(ev[0].elapsed_time(ev[1]))
        t["train_ms"].append(ev[1].elapsed_time(ev[2]))
    result["train_vs_collect"] = {"env": "HoverAviary(RPM)", "envs": envs, "n_steps": n_steps, "batch_size": batch_size,
                                  "n_epochs": n_epochs, "updates": n_epochs * ((envs * n_steps + batch_size - 1) // batch_size),
                                  "policy": "72-64-64-4", "collect_ms": float(np.median(t["collect_ms"])),
                                  "train_ms": float(np.median(t["train_ms"])), "runs": t,
                                  "note": "eager Python launches, device events around each call"}
    print(json.dumps(result["train_vs_collect"]), flush=True)
    learner.close()
    pol.close()
    env.close()


def launches(n, reps=200):
    """rocprofv3 --kernel-trace --stats target: `reps` fused updates of n rows, 72-64-64-4 (the per-launch breakdown)"""
    rng = np.random.default_rng(0)
    for in_dim, h, out in ((72, 64, 4),):
        for n in (n,):
            rows = 2 * n
            bufs = (torch.randn((rows, in_dim), device="cuda"), torch.randn((rows, out), device="cuda") * 0.5,
                    torch.randn(rows, device="cuda"), torch.randn(rows, device="cuda") * 0.3 - 0.92 * out,
                    torch.randn(rows, device="cuda"), torch.randn(rows, device="cuda"))
            idx = torch.randperm(rows, device="cuda")[:n].contiguous()
            pol = DevicePolicy(random_net(rng, in_dim, h, out), "tanh", 0, "raw")
            learner = PPOLearner(pol)
            for _ in range(reps):
                learner.update(*bufs, idx)
            torch.cuda.synchronize()
            learner.close()
            pol.close()
    print("ok")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "launches":
        launches(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
        sys.exit(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "ppo_update.json"))
    ap.add_argument("--errors", default=None)
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "updates_per_graph": INNER,
              "replays_per_round": REPLAYS, "unit": "microseconds per minibatch update, median over the rounds", "updates": []}
    updates(args, result)
    train_vs_collect(result)
    if args.errors and os.path.exists(args.errors):
        result["errors_vs_float64"] = [json.loads(line) for line in open(args.errors) if line.strip()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
