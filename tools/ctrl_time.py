"""Step-kernel time of CtrlAviary and VelocityAviary against MultiHoverAviary's at the same (E, N).

usage: python tools/ctrl_time.py [--steps 1000] [--warmup 100] [--out profiles/ctrl_kernel.json]   (one GPU)

The method of tools/multihover_time.py: per-launch kernel durations from the events attached to the step
kernel's own dispatch (adrp_profile_begin / _end), in one run, (E, N) = (4096, 1), (2048, 2), (1024, 4),
(512, 8) -- 4,096 lanes each -- for Physics.PYB and PYB_DW in fp64 and fp32, all three envs at 240 / 30 Hz
(8 sub-steps), the drones of an env 0.18 m above each other so that the downwash acts.  MultiHoverAviary
runs with auto-reset and random actions; CtrlAviary gets the RPMs of the same random actions,
VelocityAviary random velocity commands, and as neither ever ends an episode both are reset every 64
steps (a launch of its own, not timed) so that the drones stay in the air.  Prints one JSON line (and
writes it to --out): mean / median / max [us] per configuration and the ratio of the medians to
MultiHoverAviary's.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gym_pybullet_adrp_amd.envs import CtrlAviary, MultiHoverAviary, VelocityAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Physics  # noqa: E402

NOISE = {"xyz": 0.02, "rpy": 0.05, "vel": 0.1, "omega": 0.2}
RESET_EVERY = 64


def kernel_us(env, acts, steps, warmup, reset_every=0):
    env.reset()
    for k in range(warmup):
        env.step(acts[k % 16])
    torch.cuda.synchronize()
    env.h.profile_begin(steps)
    for k in range(steps):
        if reset_every and k % reset_every == 0:
            env.reset()
        env.step(acts[k % 16])
    us = np.asarray(env.h.profile_end(steps), dtype=np.float64) * 1e3
    assert len(us) == steps
    name = env.kernel_name
    env.close()
    return {"kernel": name, "mean_us": round(float(us.mean()), 3), "median_us": round(float(np.median(us)), 3),
            "max_us": round(float(us.max()), 3), "launches": int(steps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"lanes": 4096, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "runs": {}}
    g = torch.Generator(device=dev).manual_seed(0)
    kernel_us(MultiHoverAviary(num_drones=1, num_envs=4096), [torch.zeros((4096, 1, 4), device=dev)] * 16, 2000, 0)   # discarded: the clocks settle
    for prec in ("fp64", "fp32"):
        for phys in (Physics.PYB, Physics.PYB_DW):
            r = {}
            for E, N in ((4096, 1), (2048, 2), (1024, 4), (512, 8)):
                xyz = [[0.05 * n, 0.0, (1.0 if N == 1 else 0.5) + 0.18 * n] for n in range(N)]
                kw = dict(num_drones=N, num_envs=E, initial_xyzs=xyz, physics=phys, pyb_freq=240, ctrl_freq=30,
                          precision=prec, seed=1, init_noise=NOISE)
                acts = [torch.rand((E, N, 4), device=dev, generator=g) * 2 - 1 for _ in range(16)]
                m = kernel_us(MultiHoverAviary(**kw), acts, args.steps, args.warmup)
                r[f"multihover_E{E}_N{N}"] = m
                env = CtrlAviary(**kw)
                rpms = [(env.HOVER_RPM * (1 + 0.05 * a.double())).to(env.h.real) for a in acts]
                c = kernel_us(env, rpms, args.steps, args.warmup, RESET_EVERY)
                vacts = [torch.cat([a[..., :3], a[..., 3:].abs()], -1).contiguous() for a in acts]
                v = kernel_us(VelocityAviary(**kw), vacts, args.steps, args.warmup, RESET_EVERY)
                for key, x in ((f"ctrl_E{E}_N{N}", c), (f"velocity_E{E}_N{N}", v)):
                    x["ratio_to_multihover"] = round(x["median_us"] / m["median_us"], 3)
                    r[key] = x
            out["runs"][f"{prec}/{phys.name}"] = r
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
