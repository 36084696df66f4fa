"""On-device policy probes.

python tools/policy_probe.py [reps]
    launch the narrow policy forward N times per configuration (rocprofv3 --kernel-trace target)

python tools/policy_probe.py wide [--rows 4096] [--rounds 7] [--out profiles/policy_wide.json]
    time, graph-replayed, the wide `act` and `sample` launches (72 -> 4, 144 -> 8, 576 -> 32; hidden
    64 / 64, tanh) beside the narrow 49 -> 4 launch and beside the yardstick: torch's own fp32 forward
    of the same actor MLP (three F.linear + tanh) on the same rows, captured and replayed the same way.
    Every arm is one HIP graph of INNER launches; a round replays each arm's graph in turn (interleaved),
    timed with device events; the figure is the median over the rounds, the margin the torch arm's own
    round-to-round spread.  Also the step time of the env each shape drives."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_pybullet_adrp_amd.policy import ACTOR_KEYS, CRITIC_KEYS, DevicePolicy  # noqa: E402

INNER, REPLAYS = 50, 20


def narrow_launches(reps):
    g = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "policy_golden.npz"))
    for name, rows in (("example_RL_model", 4096), ("twogates", 16384)):
        w = {k: g[f"{name}_w{i}"] for i, k in enumerate(ACTOR_KEYS)}
        pol = DevicePolicy(w, "relu" if bool(g[f"{name}_relu"]) else "tanh", 0, "relative")
        obs = torch.rand((rows, 49), device="cuda") * 2 - 1
        out = torch.empty((rows, 4), device="cuda")
        for _ in range(reps):
            pol.act(obs, out=out)
        torch.cuda.synchronize()
        pol.close()
    print("ok")


def random_net(rng, in_dim, h, out):
    def lin(o, i, scale=1.0):
        return ((rng.standard_normal((o, i)) * np.sqrt(2.0 / i) * scale).astype(np.float32),
                (rng.standard_normal(o) * 0.1).astype(np.float32))
    wd = dict(zip(ACTOR_KEYS, lin(h, in_dim) + lin(h, h) + lin(out, h, 0.3)))
    wd.update(zip(CRITIC_KEYS, lin(h, in_dim) + lin(h, h) + lin(1, h, 0.3) + (rng.uniform(-1, 0, out).astype(np.float32),)))
    return wd


def graph_of(fn, stream):
    """one HIP graph of INNER calls of fn (warmed on the capture stream first)"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(INNER):
                fn()
    return g


def time_graph(g):
    """microseconds per launch over REPLAYS replays (device events around the replays)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g.replay()
    torch.cuda.synchronize()
    a.record()
    for _ in range(REPLAYS):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (REPLAYS * INNER)


def env_step_us(shape, rows):
    """eager step time of the env the shape drives (device events over 200 steps, after 20 warm-up steps)"""
    from gym_pybullet_adrp_amd.envs.hover import HoverAviary
    from gym_pybullet_adrp_amd.envs.multihover import MultiHoverAviary
    from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary
    in_dim = shape[0]
    if in_dim == 49:
        env, name = MultiRaceAviary("level0", num_drones=1, num_envs=rows, seed=1), "MultiRaceAviary(level0, 1 drone)"
    elif in_dim == 72:
        env, name = HoverAviary(num_envs=rows, seed=1, initial_xyzs=[0, 0, 1.0]), "HoverAviary(RPM)"
    else:
        n = in_dim // 72
        env, name = MultiHoverAviary(num_drones=n, num_envs=rows, seed=1), f"MultiHoverAviary({n} drones, RPM)"
    env.reset()
    act = torch.zeros(tuple(env._act_shape), device=env.device)
    for _ in range(20):
        env.step(act)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(200):
        env.step(act)
    b.record()
    torch.cuda.synchronize()
    env.close()
    return name, a.elapsed_time(b) * 1e3 / 200


def wide(args):
    import torch.nn.functional as F
    rows, rng = args.rows, np.random.default_rng(0)
    stream = torch.cuda.Stream()
    result = {"rows": rows, "rounds": args.rounds, "launches_per_graph": INNER, "replays_per_round": REPLAYS,
              "unit": "microseconds per launch, median over the rounds", "device": torch.cuda.get_device_name(0),
              "shapes": []}
    for shape in ((49, 64, 4), (72, 64, 4), (144, 64, 8), (576, 64, 32)):
        in_dim, h, out = shape
        wd = random_net(rng, *shape)
        pol = DevicePolicy(wd, "tanh", 0, "raw")
        obs = torch.rand((rows, in_dim), device="cuda") * 4 - 2
        o_act = torch.empty((rows, out), device="cuda")
        bufs = (torch.empty((rows, out), device="cuda"), torch.empty((rows, out), device="cuda"),
                torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda"))
        tw = [torch.from_numpy(wd[k]).cuda() for k in ACTOR_KEYS]

        def torch_forward():
            x = torch.tanh(F.linear(obs, tw[0], tw[1]))
            x = torch.tanh(F.linear(x, tw[2], tw[3]))
            return F.linear(x, tw[4], tw[5])
        arms = {"act": graph_of(lambda: pol.act(obs, out=o_act), stream),
                "sample": graph_of(lambda: pol.sample(obs, 1, 2, *bufs), stream),
                "torch_fp32_forward": graph_of(torch_forward, stream)}
        with torch.cuda.stream(stream):
            ref = torch_forward().clamp(-1, 1)
            pol.act(obs, out=o_act)
            torch.cuda.synchronize()
            diff = float((ref - o_act).abs().max())
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, g in arms.items():
                times[k].append(time_graph(g))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = float(max(times["torch_fp32_forward"]) - min(times["torch_fp32_forward"]))
        env_name, env_us = env_step_us(shape, rows)
        rec = {"shape": f"{in_dim}-{h}-{h}-{out}", "path": "narrow" if in_dim <= 64 and out <= 4 else "wide",
               "act_us": med["act"], "sample_us": med["sample"], "torch_us": med["torch_fp32_forward"],
               "torch_spread_us": spread, "rounds_us": times, "act_vs_torch_max_abs_diff": diff,
               "act_no_slower": med["act"] <= med["torch_fp32_forward"] + spread,
               "sample_no_slower": med["sample"] <= med["torch_fp32_forward"] + spread,
               "env": env_name, "env_step_us": env_us}
        result["shapes"].append(rec)
        print(json.dumps({k: v for k, v in rec.items() if k != "rounds_us"}), flush=True)
        pol.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "wide":
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--rows", type=int, default=4096)
        ap.add_argument("--rounds", type=int, default=7)
        ap.add_argument("--out", default=os.path.join("profiles", "policy_wide.json"))
        wide(ap.parse_args())
    else:
        narrow_launches(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
