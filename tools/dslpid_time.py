"""What the stand-alone DSLPIDControl costs a CtrlAviary loop, beside the controller fused into VelocityAviary.

usage: python tools/dslpid_time.py [--rounds 7] [--out profiles/dslpid_kernel.json]   (one GPU)

The method of tools/ppo_probe.py: every arm is one HIP graph of INNER = 20 iterations, a round replays each arm
in turn (interleaved) between device events, the figure is the median over the rounds and the margin the
round-to-round spread (max - min) of the arms.  Shapes (E, N) = (4096, 1) and (1024, 4), Physics.PYB, 240 / 48 Hz,
fp64 and fp32.  Arms, per iteration:
  a  CtrlAviary.step(rpm) + DSLPIDControl.computeControlFromState(env, target) -> rpm      two launches
  n  the same without the yaw-error output, out=(rpm, pos_e, None)                        two launches
  b  CtrlAviary.step(rpm) alone, fed fixed RPMs                                            one launch
  c  VelocityAviary.step(command)                                                          one launch
a - b is what the stand-alone controller costs a loop, c - b the controller fused into the step kernel, a - n the
yaw error (which the float32 kernel evaluates in float64, csrc/dslpid_kernel.h).
The envs are reset (not timed) before every timed run, so that the drones are in the air in every arm; arm a
uses the CF2P mixer, which holds the hover.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gym_pybullet_adrp_amd.control import DSLPIDControl  # noqa: E402
from gym_pybullet_adrp_amd.envs import CtrlAviary, VelocityAviary  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import DroneModel, Physics  # noqa: E402

INNER, REPLAYS = 20, 5


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
    """microseconds per iteration: REPLAYS replays of INNER iterations between device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prepare()
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "inner": INNER, "replays": REPLAYS, "rounds": args.rounds,
              "physics": "PYB", "pyb_freq": 240, "ctrl_freq": 48, "runs": {}}
    for precision in ("fp64", "fp32"):
        for E, N in ((4096, 1), (1024, 4)):
            xyzs = [[0.5 * n, 0.0, 1.0 + 0.2 * n] for n in range(N)]
            kw = dict(num_drones=N, initial_xyzs=xyzs, physics=Physics.PYB, pyb_freq=240, ctrl_freq=48, num_envs=E, precision=precision)
            env_a, env_n, env_b, env_c = CtrlAviary(**kw), CtrlAviary(**kw), CtrlAviary(**kw), VelocityAviary(**kw)
            ctrl = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision=precision)
            ctrl_n = DSLPIDControl(DroneModel.CF2P, num_envs=E, num_drones=N, precision=precision)
            real, dev = ctrl.real, env_a.device
            hover = torch.full((E, N, 4), float(env_a.HOVER_RPM), dtype=real, device=dev)
            rpm_a, rpm_n = hover.clone(), hover.clone()
            pos_e, yaw_e = torch.zeros((E, N, 3), dtype=real, device=dev), torch.zeros((E, N), dtype=real, device=dev)
            target = (torch.tensor(xyzs, dtype=real, device=dev)[None] + torch.from_numpy(rng.uniform(-0.05, 0.05, (E, N, 3))).to(dev, real)).contiguous()
            cmd = torch.from_numpy(rng.uniform(-1, 1, (E, N, 4)).astype(np.float32)).to(dev)
            cmd[..., 3] = cmd[..., 3].abs() * 0.2

            def prep_a():
                env_a.reset(); ctrl.reset(); rpm_a.copy_(hover)

            def arm_a():
                env_a.step(rpm_a)
                ctrl.computeControlFromState(env_a.CTRL_TIMESTEP, env_a, target, out=(rpm_a, pos_e, yaw_e))

            def prep_n():
                env_n.reset(); ctrl_n.reset(); rpm_n.copy_(hover)

            def arm_n():
                env_n.step(rpm_n)
                ctrl_n.computeControlFromState(env_n.CTRL_TIMESTEP, env_n, target, out=(rpm_n, pos_e, None))

            def arm_b():
                env_b.step(hover)

            def arm_c():
                env_c.step(cmd)
            prep = {"a": prep_a, "n": prep_n, "b": env_b.reset, "c": env_c.reset}
            graphs = {"a": graph_of(arm_a, prep_a, stream), "n": graph_of(arm_n, prep_n, stream), "b": graph_of(arm_b, env_b.reset, stream),
                      "c": graph_of(arm_c, env_c.reset, stream)}
            times = {k: [] for k in graphs}
            with torch.cuda.stream(stream):
                for _ in range(args.rounds):
                    for k, g in graphs.items():
                        times[k].append(timed(g.replay, prep[k]))
            torch.cuda.synchronize()
            assert torch.isfinite(env_a._obs).all() and torch.isfinite(rpm_a).all()
            med = {k: float(np.median(v)) for k, v in times.items()}
            spread = float(max(max(v) - min(v) for v in times.values()))
            rec = {"step_plus_controller_us": round(med["a"], 3), "step_alone_us": round(med["b"], 3),
                   "velocity_step_us": round(med["c"], 3), "standalone_controller_us": round(med["a"] - med["b"], 3),
                   "fused_controller_us": round(med["c"] - med["b"], 3),
                   "step_plus_controller_no_yaw_e_us": round(med["n"], 3), "yaw_error_us": round(med["a"] - med["n"], 3),
                   "spread_us": round(spread, 3),
                   "rounds_us": {k: [round(x, 3) for x in v] for k, v in times.items()},
                   "kernels": {"a": env_a.kernel_name + " + dslpid_control_kernel", "b": env_b.kernel_name, "c": env_c.kernel_name}}
            result["runs"][f"{precision}/E{E}_N{N}"] = rec
            print(f"{precision} E={E} N={N}: a {med['a']:.2f} b {med['b']:.2f} c {med['c']:.2f} us | a-b {med['a'] - med['b']:.2f} "
                  f"c-b {med['c'] - med['b']:.2f} a-n {med['a'] - med['n']:.2f} spread {spread:.2f}", flush=True)
            for x in (env_a, env_n, env_b, env_c, ctrl, ctrl_n):
                x.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
