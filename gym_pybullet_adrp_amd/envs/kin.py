"""What the kinematic env families share (HoverAviary; MultiHoverAviary; CtrlAviary / VelocityAviary): the
constructor's validation and ``adrp_config`` filling, the handle, the reference attributes, the output
buffers, ``reset``, ``bind_outputs``, action coercion and the introspection of the handle ``self.h``.

A subclass sets ``TASK``, checks its own observation / action types (``_check_types``), adds its task's
attributes (``_task_attributes``), builds its spaces and steps.
"""
import numpy as np
import torch

from .. import _lib
from ..utils import abi
from ..utils.enums import DroneModel, PHYSICS_CODE
from .base import AviaryEnv


def default_init_xyzs(num_drones, L=0.0397, collision_h=0.025, collision_z_offset=0.0):
    """BaseAviary.py:194-197: drone n at (4 L n, 4 L n, COLLISION_H/2 - COLLISION_Z_OFFSET + 0.1), [N, 3]"""
    return np.vstack([np.array([x * 4 * L for x in range(num_drones)]),
                      np.array([y * 4 * L for y in range(num_drones)]),
                      np.ones(num_drones) * (collision_h / 2 - collision_z_offset + .1)]).transpose().reshape(num_drones, 3)


class KinAviary(AviaryEnv):
    TASK = None        # abi.TASK_*
    HAS_TOBS = True    # terminal observations (the envs with an auto-reset); else _tobs is None

    def __init__(self, drone_model, num_drones, neighbourhood_radius, initial_xyzs, initial_rpys, physics, pyb_freq,
                 ctrl_freq, gui, record, obs=None, act=None, *, num_envs, device, precision, seed, autoreset=None,
                 init_noise, env_offset, link_frame_lag):
        """``num_drones`` None: HoverAviary, one drone whose initial pose is the config's unless given.
        ``autoreset`` None: the task has none."""
        if drone_model != DroneModel.CF2X:
            raise ValueError("only DroneModel.CF2X (cf2x_IROS.urdf) is supported")
        if gui or record:
            raise ValueError("GUI / video recording are out of scope (DESIGN.md)")
        act_code = self._check_types(obs, act)
        if pyb_freq % ctrl_freq != 0:
            raise ValueError("[ERROR] in BaseAviary.__init__(), pyb_freq is not divisible by env_freq.")
        if num_drones is not None:
            num_drones = int(num_drones)
            if not 1 <= num_drones <= abi.MAX_DRONES:
                raise ValueError(f"{type(self).__name__} num_drones must be 1..{abi.MAX_DRONES}")
        cfg = _lib.default_config(self.TASK)
        cfg.physics = PHYSICS_CODE[physics]
        cfg.num_envs = int(num_envs)
        cfg.pyb_freq, cfg.ctrl_freq = int(pyb_freq), int(ctrl_freq)
        if act_code is not None:   # the RL envs: an action type and its history
            cfg.act_type = act_code
            cfg.action_buffer_size = int(ctrl_freq // 2)
        if autoreset is not None:
            cfg.autoreset = 1 if autoreset else 0
        cfg.precision = {"fp32": 0, "fp64": 1}[precision]
        cfg.link_frame_lag = 1 if link_frame_lag else 0
        cfg.seed = int(seed) & (2 ** 64 - 1)
        cfg.env_offset = int(env_offset)
        d = cfg.drone
        if num_drones is None:
            if initial_xyzs is not None:
                abi.set_vec(cfg.init_xyz[0], np.asarray(initial_xyzs, float).reshape(3))
            if initial_rpys is not None:
                abi.set_vec(cfg.init_rpy[0], np.asarray(initial_rpys, float).reshape(3))
        else:
            cfg.num_drones = num_drones
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
            self.INIT_XYZS, self.INIT_RPYS = init_xyzs, init_rpys
            self.NEIGHBOURHOOD_RADIUS = neighbourhood_radius
        for key, dst in (("xyz", cfg.init_xyz_noise), ("rpy", cfg.init_rpy_noise), ("vel", cfg.init_vel_noise),
                         ("omega", cfg.init_omega_noise)):
            if init_noise and key in init_noise:
                abi.set_vec(dst, np.broadcast_to(np.asarray(init_noise[key], float), 3))
        self.cfg = cfg
        self.h = _lib.Handle(cfg, device)
        self.device = self.h.device
        # reference attributes
        self.DRONE_MODEL, self.PHYSICS = drone_model, physics
        if act_code is not None:
            self.OBS_TYPE, self.ACT_TYPE = obs, act
            self.ACTION_BUFFER_SIZE = int(ctrl_freq // 2)
        self.NUM_DRONES = 1 if num_drones is None else num_drones
        self.PYB_FREQ, self.CTRL_FREQ = int(pyb_freq), int(ctrl_freq)
        self.PYB_STEPS_PER_CTRL = self.PYB_FREQ // self.CTRL_FREQ
        self.PYB_TIMESTEP, self.CTRL_TIMESTEP = 1.0 / self.PYB_FREQ, 1.0 / self.CTRL_FREQ
        self.M, self.L, self.KF, self.KM = d.m, d.l, d.kf, d.km
        self.J = np.diag([d.ixx, d.iyy, d.izz])
        self.G = cfg.gravity
        self.GRAVITY = self.G * self.M
        self.HOVER_RPM = np.sqrt(self.GRAVITY / (4 * self.KF))
        self.MAX_RPM = np.sqrt((d.thrust2weight * self.GRAVITY) / (4 * self.KF))
        self._task_attributes(d)
        self.num_envs = cfg.num_envs
        self.action_space = self._actionSpace()
        self.observation_space = self._observationSpace()
        E, N = self.num_envs, self.NUM_DRONES
        self._obs = torch.zeros((E, N, self.h.D), dtype=torch.float32, device=self.device)
        self._tobs = torch.zeros_like(self._obs) if self.HAS_TOBS else None
        self._rew = torch.zeros(E, dtype=torch.float32, device=self.device)
        # the kernel writes 0/1 bytes: valid torch.bool storage, returned without a cast
        self._term = torch.zeros(E, dtype=torch.bool, device=self.device)
        self._trunc = torch.zeros(E, dtype=torch.bool, device=self.device)
        self._act_shape = (E, N, self.h.A)
        self._info = {"answer": 42}
        if self.HAS_TOBS:
            self._info["terminal_observation"] = self._tobs
        self.h.bind(self._obs, self._rew, self._term, self._trunc, self._tobs)
        self._pos_rows = None

    def _check_types(self, obs, act):
        """raise for an unsupported observation / action type; the C-ABI action code, None for an env
        without action types"""
        return None

    def _task_attributes(self, d):
        """the task's own reference attributes (``d``: the config's drone), before the spaces are built"""

    # ---- gymnasium-style API, batched ----
    def reset(self, seed: int = None, options: dict = None, mask=None):
        """Reset all envs (or those with mask[e] != 0, all drones of each); `seed` re-keys the random
        streams first.  Returns (obs [E,N,D], info)."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if seed is not None:
            # BaseAviary.reset(seed) reseeds np_random, then resets: here the Philox key of every env
            # (a fresh env built with this seed gives the same episodes from here on)
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

    def close(self):
        self.h.close()

    def bind_outputs(self, obs, rew, term, trunc, tobs=None):
        """Write step / reset outputs into caller-owned device tensors from now on (e.g. views of a
        collective's send buffer, sharding.ShardedAviary(packed=True), or the SB3 adapter's packed
        host-copy buffer): obs [E,N,D] float32, reward [E] float32, terminated / truncated [E] bool,
        optionally (an env with terminal observations) those [E,N,D] float32, all contiguous on this
        env's device."""
        if tobs is not None and not self.HAS_TOBS:
            raise TypeError(f"{type(self).__name__}.bind_outputs() takes no tobs: the env has no terminal observations")
        want = ((self._obs, obs), (self._rew, rew), (self._term, term), (self._trunc, trunc))
        if tobs is not None:
            want += ((self._tobs, tobs),)
        for old, new in want:
            if new.shape != old.shape or new.dtype != old.dtype or new.device != old.device or not new.is_contiguous():
                raise ValueError(f"bind_outputs: need a contiguous {old.dtype} {tuple(old.shape)} tensor on {old.device}")
        self._obs, self._rew, self._term, self._trunc = obs, rew, term, trunc
        if tobs is not None:
            self._tobs = tobs
            self._info["terminal_observation"] = tobs
        self.h.bind(self._obs, self._rew, self._term, self._trunc, self._tobs)

    # ---- introspection (tests / teacher forcing) ----
    def get_state(self):
        """(float [nf, E*N], int32 [ni, E*N]): the state fields, column e*N + n; the per-env ints are
        replicated on the env's columns"""
        return self.h.get_state()

    def set_state(self, f, i):
        """the per-env ints (step_counter, episode, ring_head) are taken from drone 0's column"""
        self.h.set_state(f, i)

    def state_field_names(self):
        return self.h.field_names()

    def step_bytes(self):
        return self.h.step_bytes()

    @property
    def kernel_name(self):
        """the step-kernel instantiation this env launches now (include/adrp.h adrp_handle_kernel_name)"""
        return self.h.kernel_name()
