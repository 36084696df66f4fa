"""Cost of the target_kl latch's entry check in PPOLearner.train, by device events, against another build.

python tools/ppo_train_time.py --parent PARENT_LIBADRP_SO [--rounds 7] [--repeats 5] [--out profiles/ppo_target_kl.json]

learn.py's shape: a 72-64-64-4 tanh MlpPolicy, 2,048 rows, batch 64, 10 epochs = 320 minibatch updates per train().
Three arms, interleaved round by round in rotated order, each a fresh process (ADRP_LIB picks the library of a
process) that warms up with one train() and then times --repeats more, each between two device events, and
reports their median:
  parent      target_kl=None on the library given with --parent (a build of the parent commit)
  tree        target_kl=None on this tree's library: what the entry check of the four kernels costs
  tree_trip   target_kl=0 on this tree's library: the stop trips at the first minibatch whose approx_kl is above 0,
              in the first epoch; every later launch is issued and returns at entry.  What an on-device stop costs
              where a host read per minibatch would have ended the loop.
Reported per arm: milliseconds per train(), the median and the min / max over the rounds; tree - parent beside the
parent's own round-to-round spread.  The buffers are the policy's own samples on N(0, 1) rows (old_log_prob and
old_values from the sampling launch), so the first minibatch's KL is 0 and the run is finite.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = dict(in_dim=72, hidden=64, act_dim=4, rows=2048, batch=64, epochs=10)


def child(target_kl, repeats):
    """one arm in this process -> one JSON line"""
    from types import SimpleNamespace

    import torch

    from gym_pybullet_adrp_amd.policy import DevicePolicy
    from gym_pybullet_adrp_amd.ppo import PPOLearner
    from tools.learn_hover import sb3_init

    s = SHAPE
    pol = DevicePolicy(sb3_init(s["in_dim"], s["hidden"], s["act_dim"], 0), "tanh", 0, "raw")
    learner = PPOLearner(pol, n_epochs=s["epochs"], batch_size=s["batch"], seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn((s["rows"], s["in_dim"]), device="cuda", generator=g)
    _, actions, values, log_probs = (x.clone() for x in pol.sample(obs, 0, 0))
    adv = torch.randn(s["rows"], device="cuda", generator=g)
    col = SimpleNamespace(T=s["rows"], E=1, obs=obs, actions=actions, values=values, log_probs=log_probs, advantages=adv,
                          returns=values + adv)
    learner.set_target_kl(target_kl)
    p0 = learner.state_dict()
    times = []
    for r in range(repeats + 1):                       # the first one warms up
        learner.load_state_dict(p0)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        stats = learner.train(col)
        stop.record()
        stop.synchronize()
        if r:
            times.append(start.elapsed_time(stop))
    out = {"ms": statistics.median(times), "repeats": times, "finite": bool(torch.isfinite(stats[0, 0]).all())}
    if target_kl is not None:
        out["stop_info"] = learner.stop_info()
    print("RESULT " + json.dumps(out), flush=True)
    learner.close()
    pol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libadrp.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(None if args.child == "none" else float(args.child), args.repeats)
    if not args.parent or not os.path.exists(args.parent):
        raise SystemExit("--parent: the parent commit's libadrp.so is needed for the comparison")
    arms = {"parent": (os.path.abspath(args.parent), "none"), "tree": (None, "none"), "tree_trip": (None, "0")}
    order = tuple(arms)
    results = {a: [] for a in arms}
    for r in range(args.rounds):
        for a in order[r % len(order):] + order[:r % len(order)]:      # rotate the order round by round
            lib, target = arms[a]
            env = dict(os.environ)
            env.pop("ADRP_LIB", None)
            if lib:
                env["ADRP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", target, "--repeats", str(args.repeats)],
                               env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:                          # nothing more is started on the GPU
                raise SystemExit(f"arm {a}, round {r}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            results[a].append(json.loads(line[0][len("RESULT "):]))
    ms = {a: [x["ms"] for x in v] for a, v in results.items()}
    med = {a: statistics.median(v) for a, v in ms.items()}
    out = {"shape": SHAPE, "updates_per_train": SHAPE["epochs"] * (SHAPE["rows"] // SHAPE["batch"]), "rounds": args.rounds,
           "repeats_per_process": args.repeats,
           "ms_per_train": {a: {"median": med[a], "min": min(v), "max": max(v), "rounds": v} for a, v in ms.items()},
           "tree_minus_parent_ms": med["tree"] - med["parent"],
           "parent_round_to_round_spread_ms": max(ms["parent"]) - min(ms["parent"]),
           "tree_trip_stop_info": results["tree_trip"][0]["stop_info"],
           "all_finite": all(x["finite"] for v in results.values() for x in v)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
