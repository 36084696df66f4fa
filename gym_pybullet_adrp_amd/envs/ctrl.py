"""CtrlAviary on the GPU: E independent envs of N drones each, raw motor speeds in, drone state rows out,
stepped by one fused HIP launch.

Mirrors the reference surface (envs/CtrlAviary.py, envs/BaseAviary.py): same constructor arguments and
attributes, per-env spaces of shape ``(NUM_DRONES, .)``, the action the four RPMs of every drone, clipped
to ``[0, MAX_RPM]``, the observation ``_getDroneStateVector``'s 20 floats per drone:
[pos 3, quat 4 (xyzw), rpy 3, vel 3, ang_v 3, last_clipped_action 4], the last four the RPMs applied in
this step (zero after a reset).  The reward is -1, terminated and truncated are False, always: the env
never ends an episode and there is no auto-reset.  Batched extras as MultiHoverAviary's: ``num_envs``,
``device``, ``precision``, ``seed``, ``init_noise``, ``env_offset``, ``link_frame_lag``.

The kernel runs one lane per (env, drone); with ``Physics.PYB_DW`` / ``PYB_GND_DRAG_DW`` the drones of an
env exchange positions every physics sub-step for the downwash.

Deviations: drone-drone contact is NOT modelled (``min_pair_distance()`` shows when a run
has left the modelled regime); the ground is the documented plane model, per drone; ``obstacles``,
``user_debug_gui`` and ``output_folder`` are accepted and ignored.

``step``/``reset`` take and return torch tensors that live on the GPU (no host copy): obs [E, N, 20]
float32, action [E, N, 4], reward [E] float32, terminated / truncated [E] bool.  A float64 env takes a
float64 action tensor as it is: the reference feeds float64 RPMs, and rounding them to float32 costs about
3e-5 relative in the velocity after one step.
"""
import numpy as np
import torch

from .. import _lib
from ..utils import abi
from ..utils.enums import DroneModel, Physics, PHYSICS_CODE
from ..utils.spaces import Box
from .base import AviaryEnv
from .multihover import MultiDroneHelpers, default_init_xyzs

# cf2x_IROS.urdf (adrp_default_config): what the spaces need before any handle exists
_M, _KF, _T2W, _G, _MAX_SPEED_KMH = 0.03454, 3.16e-10, 2.25, 9.8, 30.0


def max_rpm(m=_M, kf=_KF, thrust2weight=_T2W, g=_G):
    """BaseAviary.py:120: MAX_RPM = sqrt(THRUST2WEIGHT_RATIO * GRAVITY / (4 KF)), GRAVITY = G * M"""
    return np.sqrt((thrust2weight * (g * m)) / (4 * kf))


def state_row_space(num_drones, top=None):
    """observation space of CtrlAviary / VelocityAviary, shape (N, 20) (CtrlAviary.py:99-102)"""
    top = max_rpm() if top is None else top
    inf, pi = np.inf, np.pi
    lo = [-inf, -inf, 0., -1., -1., -1., -1., -pi, -pi, -pi, -inf, -inf, -inf, -inf, -inf, -inf, 0., 0., 0., 0.]
    hi = [inf, inf, inf, 1., 1., 1., 1., pi, pi, pi, inf, inf, inf, inf, inf, inf, top, top, top, top]
    return Box(low=np.array([lo] * num_drones), high=np.array([hi] * num_drones), dtype=np.float32)


def ctrl_spaces(num_drones, top=None):
    """(action_space, observation_space) of one CtrlAviary env (CtrlAviary.py:74-102)"""
    top = max_rpm() if top is None else top
    return (Box(low=np.zeros((num_drones, 4)), high=np.full((num_drones, 4), top), dtype=np.float32),
            state_row_space(num_drones, top))


class StateRowAviary(MultiDroneHelpers, AviaryEnv):
    """What CtrlAviary and VelocityAviary share: the constructor, the buffers, reset and the outputs."""

    TASK = None   # abi.TASK_CTRL / abi.TASK_VELOCITY

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, num_drones: int = 1,
                 neighbourhood_radius: float = np.inf, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.PYB, pyb_freq: int = 240, ctrl_freq: int = 240, gui=False,
                 record=False, obstacles=False, user_debug_gui=True, output_folder="results",
                 *, num_envs: int = 1, device: int = 0, precision: str = "fp64", seed: int = 0,
                 init_noise=None, env_offset: int = 0, link_frame_lag: bool = True):
        name = type(self).__name__
        if drone_model != DroneModel.CF2X:
            raise ValueError("only DroneModel.CF2X (cf2x_IROS.urdf) is supported")
        if gui or record:
            raise ValueError("GUI / video recording are out of scope (DESIGN.md)")
        if pyb_freq % ctrl_freq != 0:
            raise ValueError("[ERROR] in BaseAviary.__init__(), pyb_freq is not divisible by env_freq.")
        num_drones = int(num_drones)
        if not 1 <= num_drones <= abi.MAX_DRONES:
            raise ValueError(f"{name} num_drones must be 1..{abi.MAX_DRONES}")
        cfg = _lib.default_config(self.TASK)
        cfg.num_drones = num_drones
        cfg.physics = PHYSICS_CODE[physics]
        cfg.num_envs = int(num_envs)
        cfg.pyb_freq, cfg.ctrl_freq = int(pyb_freq), int(ctrl_freq)
        cfg.precision = {"fp32": 0, "fp64": 1}[precision]
        cfg.link_frame_lag = 1 if link_frame_lag else 0
        cfg.seed = int(seed) & (2 ** 64 - 1)
        cfg.env_offset = int(env_offset)
        d = cfg.drone
        if initial_xyzs is None:
            init_xyzs = default_init_xyzs(num_drones, d.l, d.collision_h, d.collision_z_offset)
        else:
            init_xyzs = np.asarray(initial_xyzs, float)
            if init_xyzs.shape != (num_drones, 3):
                raise ValueError("[ERROR] invalid initial_xyzs in BaseAviary.__init__(), try initial_xyzs.reshape(NUM_DRONES,3)")
        if initial_rpys is None:
            init_rpys = np.zeros((num_drones, 3))
        else:
            init_rpys = np.asarray(initial_rpys, float)
            if init_rpys.shape != (num_drones, 3):
                raise ValueError("[ERROR] invalid initial_rpys in BaseAviary.__init__(), try initial_rpys.reshape(NUM_DRONES,3)")
        for n in range(abi.MAX_DRONES):
            abi.set_vec(cfg.init_xyz[n], init_xyzs[n] if n < num_drones else np.zeros(3))
            abi.set_vec(cfg.init_rpy[n], init_rpys[n] if n < num_drones else np.zeros(3))
        for key, dst in (("xyz", cfg.init_xyz_noise), ("rpy", cfg.init_rpy_noise), ("vel", cfg.init_vel_noise),
                         ("omega", cfg.init_omega_noise)):
            if init_noise and key in init_noise:
                abi.set_vec(dst, np.broadcast_to(np.asarray(init_noise[key], float), 3))
        self.cfg = cfg
        self.h = _lib.Handle(cfg, device)
        self.device = self.h.device
        # reference attributes
        self.DRONE_MODEL, self.PHYSICS = drone_model, physics
        self.NUM_DRONES = num_drones
        self.NEIGHBOURHOOD_RADIUS = neighbourhood_radius
        self.PYB_FREQ, self.CTRL_FREQ = int(pyb_freq), int(ctrl_freq)
        self.PYB_STEPS_PER_CTRL = self.PYB_FREQ // self.CTRL_FREQ
        self.PYB_TIMESTEP, self.CTRL_TIMESTEP = 1.0 / self.PYB_FREQ, 1.0 / self.CTRL_FREQ
        self.INIT_XYZS, self.INIT_RPYS = init_xyzs, init_rpys
        self.OBSTACLES, self.USER_DEBUG, self.OUTPUT_FOLDER = obstacles, user_debug_gui, output_folder   # (ignored)
        self.M, self.L, self.KF, self.KM = d.m, d.l, d.kf, d.km
        self.J = np.diag([d.ixx, d.iyy, d.izz])
        self.G = cfg.gravity
        self.GRAVITY = self.G * self.M
        self.HOVER_RPM = np.sqrt(self.GRAVITY / (4 * self.KF))
        self.MAX_RPM = np.sqrt((d.thrust2weight * self.GRAVITY) / (4 * self.KF))
        self.MAX_SPEED_KMH = d.max_speed_kmh
        self.num_envs = cfg.num_envs
        self.action_space = self._actionSpace()
        self.observation_space = self._observationSpace()
        E, N = self.num_envs, num_drones
        self._obs = torch.zeros((E, N, self.h.D), dtype=torch.float32, device=self.device)
        self._rew = torch.zeros(E, dtype=torch.float32, device=self.device)
        # the kernel writes 0/1 bytes: valid torch.bool storage, returned without a cast
        self._term = torch.zeros(E, dtype=torch.bool, device=self.device)
        self._trunc = torch.zeros(E, dtype=torch.bool, device=self.device)
        self._act_shape = (E, N, 4)
        self._info = {"answer": 42}
        self.h.bind(self._obs, self._rew, self._term, self._trunc)
        self._pos_rows = None

    def _observationSpace(self):
        return state_row_space(self.NUM_DRONES, self.MAX_RPM)

    # ---- gymnasium-style API, batched ----
    def reset(self, seed: int = None, options: dict = None, mask=None):
        """Reset all envs (or those with mask[e] != 0, all N drones of each) to the initial poses; `seed`
        re-keys the random streams first.  Returns (obs [E,N,20], info)."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if seed is not None:
            if m is not None:
                raise ValueError("reset(seed=...) re-keys every env: call it without a mask")
            self.h.reseed(seed)
        self.h.reset(self._obs, m)
        return self._obs, {"answer": 42}

    def _as_action(self, action, dtype):
        act = action
        if not (isinstance(act, torch.Tensor) and act.dtype == dtype and act.device == self.device
                and act.is_contiguous() and act.shape == self._act_shape):
            act = torch.as_tensor(action, device=self.device, dtype=dtype).reshape(self._act_shape).contiguous()
        return act

    def step(self, action):
        """One env.step of every env: action [E,N,4] float32 (torch or numpy).

        Returns views of persistent device buffers (obs [E,N,20], reward [E], terminated [E],
        truncated [E]) that the next step overwrites."""
        self.h.step_ptr(self._as_action(action, torch.float32).data_ptr())
        return self._obs, self._rew, self._term, self._trunc, self._info

    def bind_outputs(self, obs, rew, term, trunc):
        """Write step / reset outputs into caller-owned device tensors from now on: obs [E,N,20] float32,
        reward [E] float32, terminated / truncated [E] bool, all contiguous on this env's device."""
        for old, new in ((self._obs, obs), (self._rew, rew), (self._term, term), (self._trunc, trunc)):
            if new.shape != old.shape or new.dtype != old.dtype or new.device != old.device or not new.is_contiguous():
                raise ValueError(f"bind_outputs: need a contiguous {old.dtype} {tuple(old.shape)} tensor on {old.device}")
        self._obs, self._rew, self._term, self._trunc = obs, rew, term, trunc
        self.h.bind(self._obs, self._rew, self._term, self._trunc)


class CtrlAviary(StateRowAviary):
    """Batched counterpart of gym_pybullet_adrp.envs.CtrlAviary."""

    TASK = abi.TASK_CTRL

    def _actionSpace(self):
        return ctrl_spaces(self.NUM_DRONES, self.MAX_RPM)[0]

    def step(self, action):
        """One env.step of every env: action [E,N,4], the RPMs of every motor (torch or numpy), clipped to
        [0, MAX_RPM] by the kernel.  A float64 env takes a float64 tensor unrounded; float32 RPMs are
        valid for both precisions.  Returns as StateRowAviary.step."""
        is_f32 = (isinstance(action, torch.Tensor) and action.dtype == torch.float32) or \
                 (isinstance(action, np.ndarray) and action.dtype == np.float32)
        if self.h.real == torch.float64 and not is_f32:
            self.h.step_rpm_ptr(self._as_action(action, torch.float64).data_ptr())
        else:
            self.h.step_ptr(self._as_action(action, torch.float32).data_ptr())
        return self._obs, self._rew, self._term, self._trunc, self._info
