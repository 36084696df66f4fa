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

from ..utils import abi
from ..utils.enums import DroneModel, Physics
from ..utils.spaces import Box
from .kin import KinAviary
from .multihover import MultiDroneHelpers

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


class StateRowAviary(MultiDroneHelpers, KinAviary):
    """What CtrlAviary and VelocityAviary share: the state-row observation and the float32 step.  No action
    types, no auto-reset, no terminal observations."""

    TASK = None   # abi.TASK_CTRL / abi.TASK_VELOCITY
    HAS_TOBS = False

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, num_drones: int = 1,
                 neighbourhood_radius: float = np.inf, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.PYB, pyb_freq: int = 240, ctrl_freq: int = 240, gui=False,
                 record=False, obstacles=False, user_debug_gui=True, output_folder="results",
                 *, num_envs: int = 1, device: int = 0, precision: str = "fp64", seed: int = 0,
                 init_noise=None, env_offset: int = 0, link_frame_lag: bool = True):
        super().__init__(drone_model, num_drones, neighbourhood_radius, initial_xyzs, initial_rpys, physics, pyb_freq,
                         ctrl_freq, gui, record, num_envs=num_envs, device=device, precision=precision, seed=seed,
                         init_noise=init_noise, env_offset=env_offset, link_frame_lag=link_frame_lag)
        self.OBSTACLES, self.USER_DEBUG, self.OUTPUT_FOLDER = obstacles, user_debug_gui, output_folder   # (ignored)

    def _task_attributes(self, d):
        self.MAX_SPEED_KMH = d.max_speed_kmh

    def _observationSpace(self):
        return state_row_space(self.NUM_DRONES, self.MAX_RPM)

    # ---- gymnasium-style API, batched (reset, bind_outputs: KinAviary) ----
    def step(self, action):
        """One env.step of every env: action [E,N,4] float32 (torch or numpy).

        Returns views of persistent device buffers (obs [E,N,20], reward [E], terminated [E],
        truncated [E]) that the next step overwrites."""
        self.h.step_ptr(self._as_action(action, torch.float32).data_ptr())
        return self._obs, self._rew, self._term, self._trunc, self._info


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
