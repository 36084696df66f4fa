"""The drone camera of the race scene: depth, segmentation and colour images on the GPU.

``BaseAviary._getDroneImages`` (BaseAviary.py:569-621) for E envs x N drones in one launch
(include/adrp.h ``adrp_race_camera``; csrc/camera_core.h): every pixel casts one ray against the
scene's analytic shapes: the ground plane, the gates' and obstacles' URDF boxes and cylinders at the
env's own poses, and the env's other drones as their collision cylinders.  DESIGN.md §3.19 states the
camera model (pybullet's documented view / projection / depth-buffer conventions) and the deviations:
an unlit albedo image, cylinders for the other drones, the camera's own drone not drawn, a primitive
entered before the near plane not seen.

    cam = DroneCamera(env, width=64, height=48)
    img = cam.render()            # {"rgb": uint8 [E,N,H,W,4], "dep": float32 [E,N,H,W], "seg": int32 [E,N,H,W]}
    z = linear_depth(img["dep"])  # eye-space depth in metres

``render`` returns the same device tensors on every call and does not synchronise.
"""
import ctypes

import torch

from . import _lib
from .utils import abi

ARM = 0.0397                 # cf2x arm: eye = pos + (0, 0, ARM); the near plane
NEAR, FAR = ARM, 1000.0
IMG_FRAME_PER_SEC = 24       # BaseAviary.py:136
OUTPUTS = ("rgb", "dep", "seg")
CAPTURES = ("always", "reference")


def linear_depth(dep):
    """eye-space depth [m] of depth-buffer values (tensor or ndarray): far near / (far - (far - near) dep)"""
    return FAR * NEAR / (FAR - (FAR - NEAR) * dep)


class DroneCamera:
    """Camera of every drone of a ``MultiRaceAviary`` (or, through ``render_poses``, of constructed poses).

    ``outputs``: which of "rgb", "dep", "seg" are rendered.  ``capture``: "always" renders every
    (env, drone) at every call; "reference" only those whose ``step_counter`` is a multiple of
    ``PYB_FREQ // 24`` (the reference's IMG_CAPTURE_FREQ test), the other images keep their last
    content (zeros / ones / minus ones before the first capture)."""

    def __init__(self, env, width=64, height=48, outputs=OUTPUTS, capture="always"):
        outputs = tuple(outputs)
        if not outputs or any(o not in OUTPUTS for o in outputs):
            raise ValueError(f"outputs must be a non-empty subset of {OUTPUTS}, not {outputs!r}")
        if capture not in CAPTURES:
            raise ValueError(f"capture must be one of {CAPTURES}, not {capture!r}")
        if int(width) < 1 or int(height) < 1:
            raise ValueError("width and height must be at least 1")
        h = getattr(env, "h", None)
        if h is None or getattr(env, "cfg", None) is None or env.cfg.task != abi.TASK_RACE:
            raise ValueError("DroneCamera renders the race scene: env must be a MultiRaceAviary")
        self.env, self.lib = env, _lib.load()
        self.device = env.device
        self.E, self.N, self.W, self.H = int(env.num_envs), int(env.NUM_DRONES), int(width), int(height)
        if self.E * self.N * self.H * self.W > 2 ** 31 - 1:
            raise ValueError("num_envs * num_drones * height * width is past 2^31 - 1")
        self.outputs, self.capture = outputs, capture
        self.capture_freq = int(env.PYB_FREQ) // IMG_FRAME_PER_SEC if capture == "reference" else 0
        shape = (self.E, self.N, self.H, self.W)
        self.images = {}
        if "rgb" in outputs:
            self.images["rgb"] = torch.zeros(shape + (4,), dtype=torch.uint8, device=self.device)
        if "dep" in outputs:
            self.images["dep"] = torch.ones(shape, dtype=torch.float32, device=self.device)
        if "seg" in outputs:
            self.images["seg"] = torch.full(shape, -1, dtype=torch.int32, device=self.device)
        t = env.cfg.track
        self.num_gates, self.num_obstacles = int(t.num_gates), int(t.num_obstacles)
        self.gate_low = [int(t.gates[g][6] > 0) for g in range(4)]
        self._io = self._make_io(self.E, self.N, self.images, self.capture_freq)
        self._dev_index = self.device.index

    def _make_io(self, E, N, images, capture_freq):
        io = abi.AdrpRaceCameraIO()
        io.struct_size = ctypes.sizeof(abi.AdrpRaceCameraIO)
        io.num_envs, io.num_drones, io.width, io.height = E, N, self.W, self.H
        io.capture_freq = capture_freq
        for k in OUTPUTS:
            setattr(io, k, images[k].data_ptr() if k in images else None)
        return io

    def __getattr__(self, name):
        if name in OUTPUTS and name in self.__dict__.get("images", {}):
            return self.images[name]
        raise AttributeError(name)

    def _mask(self, mask, E):
        if mask is None:
            return None
        m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if m.numel() != E:
            raise ValueError(f"mask must have {E} elements")
        return m

    def render(self, mask=None):
        """Render from the env's current state (one launch on the caller's current stream) and return
        the dict of image tensors; ``mask`` [E]: only the envs with a non-zero entry."""
        m = self._mask(mask, self.E)
        io = self._io
        io.mask = None if m is None else m.data_ptr()
        rc = self.lib.adrp_race_camera_env(ctypes.byref(io), self.env.h.h, _lib._raw_stream(self._dev_index))
        if rc != 0:
            raise _lib.AdrpError(self.lib.adrp_last_error(None).decode())
        return self.images

    def render_poses(self, pos, quat, gates, obstacles, gate_low=None, num_gates=None, num_obstacles=None,
                     step_counter=None, capture_freq=0, mask=None, out=None):
        """The handle-less path for constructed poses: SoA planes as ``get_state`` lays them out, float32
        or float64 device tensors: pos [3, E*N], quat [4, E*N] (x, y, z, w), gates [16, E*N] (x, y, z,
        yaw of gate 0..3), obstacles [12, E*N]; E*N must be a multiple of this camera's N.  The scene
        (gate types, counts) defaults to the env's track.  Renders into ``out`` (a dict of tensors like
        ``images``) or into fresh tensors, and returns that dict."""
        dt = pos.dtype
        if dt not in (torch.float32, torch.float64):
            raise ValueError("state planes must be float32 or float64")
        EN = int(pos.shape[-1])
        if EN % self.N:
            raise ValueError(f"E*N = {EN} is not a multiple of num_drones = {self.N}")
        E = EN // self.N
        planes = []
        for name, t, rows in (("pos", pos, 3), ("quat", quat, 4), ("gates", gates, 16), ("obstacles", obstacles, 12)):
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == dt and t.is_contiguous()
                    and tuple(t.shape) == (rows, EN)):
                raise ValueError(f"{name} must be a contiguous {dt} [{rows}, {EN}] tensor on {self.device}")
            planes.append(t)
        if out is None:
            shape = (E, self.N, self.H, self.W)
            out = {}
            if "rgb" in self.outputs:
                out["rgb"] = torch.zeros(shape + (4,), dtype=torch.uint8, device=self.device)
            if "dep" in self.outputs:
                out["dep"] = torch.ones(shape, dtype=torch.float32, device=self.device)
            if "seg" in self.outputs:
                out["seg"] = torch.full(shape, -1, dtype=torch.int32, device=self.device)
        io = self._make_io(E, self.N, out, int(capture_freq))
        io.num_gates = self.num_gates if num_gates is None else int(num_gates)
        io.num_obstacles = self.num_obstacles if num_obstacles is None else int(num_obstacles)
        for g, low in enumerate(self.gate_low if gate_low is None else gate_low):
            io.gate_low[g] = int(low)
        io.precision = int(dt == torch.float64)
        io.pos, io.quat, io.gates, io.obstacles = (t.data_ptr() for t in planes)
        sc = None
        if step_counter is not None:
            sc = torch.as_tensor(step_counter, device=self.device).to(torch.int32).contiguous()
            if sc.numel() != EN:
                raise ValueError(f"step_counter must have {EN} elements")
            io.step_counter = sc.data_ptr()
        m = self._mask(mask, E)
        io.mask = None if m is None else m.data_ptr()
        rc = self.lib.adrp_race_camera(ctypes.byref(io), _lib._raw_stream(self._dev_index))
        if rc != 0:
            raise _lib.AdrpError(self.lib.adrp_last_error(None).decode())
        return out
