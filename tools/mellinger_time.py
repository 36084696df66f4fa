"""What the stand-alone MellingerControl costs: one compute call, and one CtrlAviary + MellingerControl loop iteration.

usage: python tools/mellinger_time.py [--rows 8192] [--replays 200] [--out profiles/mellinger_kernel.json]   (one GPU)

The method of tools/dslpid_time.py: every arm is one HIP graph of INNER = 20 iterations, replayed between device
events; the arms are interleaved replay by replay, the figure is the median over the replays (after warm-up replays
that are not counted) and the spread the 10th to 90th percentile.  rows = E x 1 controllers, Physics.PYB, 500 / 500 Hz,
fp64 and fp32.  Arms, per iteration:
  k  MellingerControl.computeControl(pos, rpy, vel) on fixed packed inputs                  one launch
  a  CtrlAviary.step(rpm) + MellingerControl.computeControlFromState(env) -> rpm           two launches
  b  CtrlAviary.step(rpm) alone, fed fixed RPMs                                            one launch
a - b is what the controller costs a loop.  The envs and controllers are reset (not timed) before every replay, so
every replay flies the same 20 ticks from the start: a FULLSTATE setpoint 0.5 m above it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gym_pybullet_adrp_amd.control import MellingerControl  # noqa: E402
from gym_pybullet_adrp_amd.control.MellingerControl import pack_command  # noqa: E402
from gym_pybullet_adrp_amd.envs import CtrlAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import Command, Physics  # noqa: E402

INNER, WARMUP = 20, 20


def graph_of(fn, prepare, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        prepare()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(INNER):
                fn()
    return g


def timed(run, prepare):
    """microseconds per iteration of one replay of INNER iterations, between device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prepare()
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    E, N = args.rows, 1
    stream = torch.cuda.Stream()
    result = {"device": torch.cuda.get_device_name(0), "rows": E * N, "inner": INNER, "warmup_replays": WARMUP,
              "replays": args.replays, "physics": "PYB", "pyb_freq": 500, "ctrl_freq": 500, "runs": {}}
    z = np.zeros(3)
    for precision in ("fp64", "fp32"):
        kw = dict(num_drones=N, initial_xyzs=[[0.0, 0.0, 1.0]], physics=Physics.PYB, pyb_freq=500, ctrl_freq=500, num_envs=E,
                  precision=precision)
        env_a, env_b = CtrlAviary(**kw), CtrlAviary(**kw)
        ctl_a = MellingerControl(num_envs=E, num_drones=N, precision=precision)
        ctl_k = MellingerControl(num_envs=E, num_drones=N, precision=precision)
        real, dev = ctl_a.real, env_a.device
        hover = torch.full((E, N, 4), float(env_a.HOVER_RPM), dtype=real, device=dev)
        rpm_a, rpm_k = hover.clone(), hover.clone()
        env_a.reset()
        rows = env_a._obs.to(real)
        pos, rpy, vel = rows[..., 0:3].contiguous(), rows[..., 7:10].contiguous(), rows[..., 10:13].contiguous()
        codes, cargs = (torch.from_numpy(x).to(dev) for x in
                        pack_command(Command.FULLSTATE, [[0.0, 0.0, 1.5], z, z, 0.0, z, 0.0], E, N))

        def prep_a():
            env_a.reset(); ctl_a.reset(env_a); ctl_a.command(codes, cargs); rpm_a.copy_(hover)

        def arm_a():
            env_a.step(rpm_a)
            ctl_a.computeControlFromState(env_a.CTRL_TIMESTEP, env_a, out=rpm_a)

        def prep_k():
            ctl_k.reset(rows); ctl_k.command(codes, cargs)

        def arm_k():
            ctl_k.computeControl(0.002, pos, rpy, vel, out=rpm_k)

        def arm_b():
            env_b.step(hover)
        prep = {"k": prep_k, "a": prep_a, "b": env_b.reset}
        graphs = {"k": graph_of(arm_k, prep_k, stream), "a": graph_of(arm_a, prep_a, stream), "b": graph_of(arm_b, env_b.reset, stream)}
        times = {k: [] for k in graphs}
        with torch.cuda.stream(stream):
            for r in range(WARMUP + args.replays):
                for k, g in graphs.items():
                    t = timed(g.replay, prep[k])
                    if r >= WARMUP:
                        times[k].append(t)
        torch.cuda.synchronize()
        assert torch.isfinite(env_a._obs).all() and torch.isfinite(rpm_a).all() and torch.isfinite(rpm_k).all()
        med = {k: float(np.median(v)) for k, v in times.items()}
        p10 = {k: float(np.percentile(v, 10)) for k, v in times.items()}
        p90 = {k: float(np.percentile(v, 90)) for k, v in times.items()}
        rec = {"compute_us": round(med["k"], 3), "step_plus_controller_us": round(med["a"], 3), "step_alone_us": round(med["b"], 3),
               "controller_in_loop_us": round(med["a"] - med["b"], 3),
               "p10_us": {k: round(v, 3) for k, v in p10.items()}, "p90_us": {k: round(v, 3) for k, v in p90.items()},
               "kernels": {"k": "mellinger_compute_kernel", "a": env_a.kernel_name + " + mellinger_compute_kernel", "b": env_b.kernel_name}}
        result["runs"][f"{precision}/rows{E * N}"] = rec
        print(f"{precision} rows={E * N}: compute {med['k']:.2f} us [{p10['k']:.2f}, {p90['k']:.2f}] | step + controller {med['a']:.2f} "
              f"[{p10['a']:.2f}, {p90['a']:.2f}] | step alone {med['b']:.2f} [{p10['b']:.2f}, {p90['b']:.2f}] | a - b {med['a'] - med['b']:.2f}", flush=True)
        for x in (env_a, env_b, ctl_a, ctl_k):
            x.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
