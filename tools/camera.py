"""Frames of the drone camera along the scripted racer's flight.

python tools/camera.py [--config getting_started] [--steps 400] [--every 10] [--out results/camera]

Flies HardCodedCommander on the track (one env, two drones), renders drone 0's camera of env 0 after every
`every`-th step and writes, per frame, the colour image, the linear depth (clipped at 5 m) and the segmentation
side by side as frame_NNNN.png (matplotlib), and all frames as rgb.npy [F, 48, 64, 4] uint8, dep.npy [F, 48, 64]
float32 (depth-buffer values) and seg.npy [F, 48, 64] int32.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_pybullet_adrp_amd.camera import DroneCamera, linear_depth  # noqa: E402
from gym_pybullet_adrp_amd.envs.race import MultiRaceAviary  # noqa: E402
from gym_pybullet_adrp_amd.hardcoded import HardCodedCommander  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="getting_started")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--out", default=os.path.join("results", "camera"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("camera: no HIP device visible; the camera has no CPU path")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    os.makedirs(a.out, exist_ok=True)
    env = MultiRaceAviary(a.config, num_drones=2, num_envs=1, seed=1, autoreset=False)
    cam = DroneCamera(env, a.width, a.height)
    obs, _ = env.reset()
    hc = HardCodedCommander(obs)
    frames = {"rgb": [], "dep": [], "seg": []}
    for k in range(a.steps):
        _, _, term, trunc, _ = env.step(hc.predict(k / env.CTRL_FREQ))
        if k % a.every == 0:
            img = cam.render()
            for key in frames:
                frames[key].append(img[key][0, 0].cpu().numpy())
        if bool(term.any()) or bool(trunc.any()):
            break
    for key, v in frames.items():
        np.save(os.path.join(a.out, f"{key}.npy"), np.stack(v))
    for n, (rgb, dep, seg) in enumerate(zip(frames["rgb"], frames["dep"], frames["seg"])):
        fig, ax = plt.subplots(1, 3, figsize=(9, 2.6))
        ax[0].imshow(rgb[..., :3])                       # (alpha 0 where nothing is hit: shown black)
        ax[0].set_title("rgb (albedo)")
        ax[1].imshow(np.minimum(linear_depth(dep.astype(np.float64)), 5.0), cmap="viridis")
        ax[1].set_title("depth [m], clipped at 5")
        ax[2].imshow(np.where(seg < 0, -1, (seg & 0xFFFFFF) * 8 + (seg >> 24)), cmap="tab20", interpolation="nearest")
        ax[2].set_title("segmentation")
        for x in ax:
            x.axis("off")
        fig.tight_layout()
        fig.savefig(os.path.join(a.out, f"frame_{n:04d}.png"), dpi=110)
        plt.close(fig)
    print(f"camera: {len(frames['rgb'])} frames of drone 0 in {a.out} ({a.config}, {k + 1} steps)")
    env.close()


if __name__ == "__main__":
    main()
