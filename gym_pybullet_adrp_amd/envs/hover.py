"""HoverAviary on the GPU: E independent envs stepped by one fused HIP launch.

Mirrors the reference surface (envs/HoverAviary.py:11-117, envs/BaseRLAviary.py,
envs/BaseAviary.py): same constructor arguments and attributes, same per-env
observation/action spaces, same obs layout [pos, rpy, vel, ang_v, 15 past actions],
reward max(0, 2-|p-(0,0,1)|^4), terminated |p-target|<1e-4, truncated by bounds / tilt /
8 s.  Batched extras: ``num_envs``, ``device``, ``precision``, ``seed``, ``autoreset``
and ``init_noise`` (per-reset uniform perturbation of the initial state, 0 = reference).
``precision`` defaults to ``"fp64"`` (the reference integrates in float64; held to 1e-9 of the
float64 CPU restatement per env.step); ``"fp32"`` is the faster float32 kernel, held to the north
star's 1e-4.

``step``/``reset`` take and return torch tensors that live on the GPU (no host copy):
obs [E, 1, D] float32, reward [E] float32, terminated / truncated [E] bool.
"""
import numpy as np
import torch

from .. import _lib
from ..utils import abi
from ..utils.enums import ActionType, DroneModel, ObservationType, Physics
from ..utils.spaces import Box
from .kin import KinAviary


# ActionType -> C-ABI code, and the per-drone action width (BaseRLAviary.py:141-147).  PID /
# VEL / ONE_D_PID run DSLPIDControl (control/DSLPIDControl.py) fused into the step kernel; its
# state persists across resets, as the reference builds the controllers once (:73-78).
_ACT_CODE = {ActionType.RPM: abi.ACT_RPM, ActionType.ONE_D_RPM: abi.ACT_ONE_D_RPM, ActionType.PID: abi.ACT_PID,
             ActionType.VEL: abi.ACT_VEL, ActionType.ONE_D_PID: abi.ACT_ONE_D_PID}
_ACT_SIZE = {ActionType.RPM: 4, ActionType.VEL: 4, ActionType.PID: 3, ActionType.ONE_D_RPM: 1,
             ActionType.ONE_D_PID: 1}


class HoverAviary(KinAviary):
    """Batched counterpart of gym_pybullet_adrp.envs.HoverAviary."""

    TASK = abi.TASK_HOVER

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.PYB, pyb_freq: int = 240, ctrl_freq: int = 30, gui=False,
                 record=False, obs: ObservationType = ObservationType.KIN, act: ActionType = ActionType.RPM,
                 *, num_envs: int = 1, device: int = 0, precision: str = "fp64", seed: int = 0,
                 autoreset: bool = True, init_noise=None, env_offset: int = 0, link_frame_lag: bool = True):
        super().__init__(drone_model, None, None, initial_xyzs, initial_rpys, physics, pyb_freq, ctrl_freq, gui, record,
                         obs, act, num_envs=num_envs, device=device, precision=precision, seed=seed, autoreset=autoreset,
                         init_noise=init_noise, env_offset=env_offset, link_frame_lag=link_frame_lag)
        self._act_ok = (None, 0)        # (tensor, address) of the last validated action

    def _check_types(self, obs, act):
        if obs != ObservationType.KIN:
            raise ValueError("only ObservationType.KIN is supported")
        if act not in _ACT_CODE:
            raise ValueError("supported action types: RPM, ONE_D_RPM, PID, VEL, ONE_D_PID")
        return _ACT_CODE[act]

    def _task_attributes(self, d):
        self.TARGET_POS = np.array([0, 0, 1])
        self.EPISODE_LEN_SEC = 8
        if self.ACT_TYPE == ActionType.VEL:
            self.SPEED_LIMIT = 0.03 * d.max_speed_kmh * (1000 / 3600)   # BaseRLAviary.py:94-95

    # ---- spaces (BaseRLAviary.py:132-156, 243-277) ----
    def _actionSpace(self):
        size = _ACT_SIZE[self.ACT_TYPE]
        return Box(low=-np.ones((1, size)), high=np.ones((1, size)), dtype=np.float32)

    def _observationSpace(self):
        lo, hi = -np.inf, np.inf
        low = [lo, lo, 0] + [lo] * 9
        high = [hi] * 12
        size = _ACT_SIZE[self.ACT_TYPE]
        low += [-1] * size * self.ACTION_BUFFER_SIZE
        high += [+1] * size * self.ACTION_BUFFER_SIZE
        return Box(low=np.array([low]), high=np.array([high]), dtype=np.float32)

    # ---- gymnasium-style API, batched (reset, bind_outputs: KinAviary) ----
    def step(self, action):
        """One env.step of every env: action [E,1,A] (torch or numpy, in [-1,1]).

        Returns views of persistent device buffers (obs [E,1,D], reward [E],
        terminated [E], truncated [E]) that the next step overwrites."""
        ok, ptr = self._act_ok
        if action is ok and action.data_ptr() == ptr:      # the tensor validated last time, unchanged
            self.h.step_ptr(ptr)
            return self._obs, self._rew, self._term, self._trunc, self._info
        act = action
        if not (isinstance(act, torch.Tensor) and act.dtype == torch.float32 and act.device == self.device
                and act.is_contiguous() and act.shape == self._act_shape):
            act = torch.as_tensor(action, device=self.device, dtype=torch.float32).reshape(self._act_shape)
            act = act.contiguous()
        else:
            self._act_ok = (action, action.data_ptr())
        self.h.step_ptr(act.data_ptr())
        return self._obs, self._rew, self._term, self._trunc, self._info

    # ---- persistent stepping (BASELINE config 1: a Python loop stepping a few envs synchronously) ----
    def persistent(self):
        """A resident step kernel for this env (include/adrp.h adrp_persistent_*): ``step(action)``
        takes a numpy action, returns numpy views of host-mapped outputs, with no kernel launch per
        step.  Use as a context manager; ``step`` / ``reset`` / ``get_state`` of the env itself are
        refused until it is closed."""
        return PersistentStepper(self)


class PersistentStepper:
    """HoverAviary.persistent(): the env.step of a resident kernel polling a host-mapped mailbox.

    ``step(action)`` writes the action (numpy, [E,1,A]) into mapped memory and returns when the
    step is done: (obs [E,1,D], reward [E], terminated [E], truncated [E], info) as numpy views of
    mapped memory that the next step overwrites (``info["terminal_observation"]`` likewise, for the
    auto-reset envs).  Results are those of ``HoverAviary.step`` on the same state and action."""

    def __init__(self, env):
        import ctypes
        self.env = env
        h = env.h
        ptrs = [ctypes.c_void_p() for _ in range(6)]
        rc = h.lib.adrp_persistent_begin(h.h, *[ctypes.byref(p) for p in ptrs])
        if rc != 0:
            raise _lib.AdrpError(f"adrp_persistent_begin: {h.lib.adrp_last_error(h.h).decode()}")
        E, D, A = env.num_envs, h.D, h.A

        def view(p, ctype, shape):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=shape)
        self.act = view(ptrs[0], ctypes.c_float, (E, 1, A))
        self.obs = view(ptrs[1], ctypes.c_float, (E, 1, D))
        self.rew = view(ptrs[2], ctypes.c_float, (E,))
        self.term = view(ptrs[3], ctypes.c_uint8, (E,)).view(np.bool_)
        self.trunc = view(ptrs[4], ctypes.c_uint8, (E,)).view(np.bool_)
        self.tobs = view(ptrs[5], ctypes.c_float, (E, 1, D))
        self.info = {"answer": 42, "terminal_observation": self.tobs}
        self._step, self._h, self._lib = h.lib.adrp_persistent_step, h.h, h.lib
        self.active = True

    def step(self, action):
        self.act[...] = action
        if self._step(self._h) != 0:
            raise _lib.AdrpError(f"adrp_persistent_step: {self._lib.adrp_last_error(self._h).decode()}")
        return self.obs, self.rew, self.term, self.trunc, self.info

    def close(self):
        if self.active:
            self.active = False
            if getattr(self.env.h, "h", None) is None:   # the env was closed first: adrp_destroy ended it
                return
            if self._lib.adrp_persistent_end(self._h) != 0:
                raise _lib.AdrpError(f"adrp_persistent_end: {self._lib.adrp_last_error(self._h).decode()}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
