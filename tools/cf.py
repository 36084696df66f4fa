"""The Crazyflie firmware-in-the-loop flight of the reference's examples/cf.py, batched on the device.

usage: python tools/cf.py [--num_envs 64] [--num_drones 1] [--takeoff] [--precision fp64] [--output_folder results]

CtrlAviary(pyb_freq=500, ctrl_freq=500) is the body, control.MellingerControl the firmware, stepped once per
physics step.  The flight: three seconds on the spot, a climb to 1 m, a square of side 1 m at that height, back to
the start column and down, every leg 75 setpoints at 25 Hz (one FULLSTATE command every 20 firmware ticks), the yaw
setpoint turning a quarter turn per leg, each drone around its own start.  --takeoff flies the climb, the corners and
the descent with the high-level commander instead (TAKEOFF, GOTO per corner, LAND; a land command finds the planner
stopped, so the drone then holds the last setpoint: control/MellingerControl.py).

Prints the final positions and writes the reference Logger's npz for the drones of env 0 (logger.DeviceLogger).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gym_pybullet_adrp_amd.control import MellingerControl  # noqa: E402
from gym_pybullet_adrp_amd.envs import CtrlAviary  # noqa: E402
from gym_pybullet_adrp_amd.logger import DeviceLogger  # noqa: E402
from gym_pybullet_adrp_amd.utils.enums import DroneModel, Physics  # noqa: E402

FIRMWARE_HZ, SETPOINT_HZ, LEG = 500, 25, 75
CORNERS = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0]], float)


def setpoints():
    """[7 * LEG, 3]: leg k runs from CORNERS[k] to CORNERS[k + 1] in LEG equal steps (the end point excluded)"""
    s = np.arange(LEG)[:, None] / LEG
    return np.concatenate([CORNERS[k] + s * (CORNERS[k + 1] - CORNERS[k]) for k in range(len(CORNERS) - 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=1)
    ap.add_argument("--num_drones", type=int, default=1)
    ap.add_argument("--takeoff", action="store_true", help="fly with the commander's TAKEOFF / GOTO / LAND")
    ap.add_argument("--precision", default="fp64", choices=["fp32", "fp64"])
    ap.add_argument("--output_folder", default="results")
    args = ap.parse_args()
    E, N = args.num_envs, args.num_drones
    start = np.array([[0.5 * n, 0.5 * n, 0.1] for n in range(N)])
    env = CtrlAviary(DroneModel.CF2X, num_drones=N, initial_xyzs=start, physics=Physics.PYB, pyb_freq=FIRMWARE_HZ,
                     ctrl_freq=FIRMWARE_HZ, num_envs=E, precision=args.precision)
    ctl = MellingerControl(DroneModel.CF2X, num_envs=E, num_drones=N, precision=args.precision)
    path = setpoints()
    every = FIRMWARE_HZ // SETPOINT_HZ
    logger = DeviceLogger(env, SETPOINT_HZ, output_folder=args.output_folder, duration_steps=len(path))
    env.reset()
    ctl.reset(env)
    zero = np.zeros(3)
    origin = start * [1.0, 1.0, 0.0]
    leg_s = LEG / SETPOINT_HZ
    for k, target in enumerate(path):
        t = k / SETPOINT_HZ
        leg, first = divmod(k, LEG)
        if not args.takeoff:
            ctl.sendFullStateCmd(np.broadcast_to(origin + target, (E, N, 3)), zero, zero, k * np.pi / (2 * LEG), zero, t)
        elif first == 0:
            if leg == 0:     # hold the start until the take-off (before any command the setpoint is the zeroed one)
                ctl.sendFullStateCmd(np.broadcast_to(start, (E, N, 3)), zero, zero, 0.0, zero, t)
            elif leg == 1:
                ctl.sendTakeoffCmd(1.0, leg_s, timestep=t)
            elif leg == 6:
                ctl.sendLandCmd(0.0, leg_s, timestep=t)
            else:
                ctl.sendGotoCmd(np.broadcast_to(origin + CORNERS[leg + 1], (E, N, 3)), 0.0, leg_s, False, timestep=t)
        for _ in range(every):
            env.step(ctl.computeControlFromState(env.CTRL_TIMESTEP, env))
        logger.log(t)
    pos = env._obs[..., 0:3].double().cpu().numpy()
    assert np.isfinite(pos).all()
    end = origin + (CORNERS[-2] if args.takeoff else path[-1])
    print(f"{E} x {N} drones, {len(path) * every} firmware ticks ({'commander' if args.takeoff else 'FULLSTATE'} flight, {args.precision})")
    for n in range(N):
        print(f"  drone {n}: final position of env 0 {np.round(pos[0, n], 4).tolist()}, last setpoint {np.round(end[n], 4).tolist()}, "
              f"largest distance to it over the envs {np.linalg.norm(pos[:, n] - end[n], axis=-1).max():.4f} m")
    print("log:", logger.save())
    env.close()
    ctl.close()


if __name__ == "__main__":
    main()
