"""MultiHoverAviary on the GPU: E independent envs of N drones each, stepped by one fused HIP launch.

Mirrors the reference surface (envs/MultiHoverAviary.py:11-130, envs/BaseRLAviary.py,
envs/BaseAviary.py): same constructor arguments and attributes, per-env spaces of shape
``(NUM_DRONES, .)``, per-drone obs rows [pos, rpy, vel, ang_v, 15 past actions of this drone],
``TARGET_POS[n] = INIT_XYZS[n] + (0, 0, 1/(n+1))``, reward sum_n max(0, 2-|target_n-p_n|^4),
terminated when sum_n |target_n-p_n| < 1e-4, truncated when any drone leaves |x|,|y| <= 2, z <= 2,
|roll|,|pitch| <= 0.4 or after 8 s.  Batched extras as HoverAviary's: ``num_envs``, ``device``,
``precision``, ``seed``, ``autoreset``, ``init_noise``, ``env_offset``, ``link_frame_lag``.

The kernel runs one lane per (env, drone); with ``Physics.PYB_DW`` / ``PYB_GND_DRAG_DW`` the drones
of an env exchange positions every physics sub-step for the downwash.

Deviations: drone-drone contact is NOT modelled (Bullet would resolve it; at the
default spacing of 0.22 m between 0.06 m-radius cylinders drones can touch) -- ``min_pair_distance()``
shows when a run has left the modelled regime; the ground is the documented plane model, per drone;
an env's drones reset together and the action history of a reset env is cleared.  Action types
PID / VEL / ONE_D_PID are not supported by this env.

``step``/``reset`` take and return torch tensors that live on the GPU (no host copy):
obs [E, N, D] float32, action [E, N, A], reward [E] float32, terminated / truncated [E] bool.
"""
import numpy as np
import torch

from .. import _lib
from ..utils import abi
from ..utils.enums import ActionType, DroneModel, ObservationType, Physics, PHYSICS_CODE
from ..utils.spaces import Box
from .base import AviaryEnv

_ACT_CODE = {ActionType.RPM: abi.ACT_RPM, ActionType.ONE_D_RPM: abi.ACT_ONE_D_RPM}
_ACT_SIZE = {ActionType.RPM: 4, ActionType.ONE_D_RPM: 1}


def default_init_xyzs(num_drones, L=0.0397, collision_h=0.025, collision_z_offset=0.0):
    """BaseAviary.py:194-197: drone n at (4 L n, 4 L n, COLLISION_H/2 - COLLISION_Z_OFFSET + 0.1), [N, 3]"""
    return np.vstack([np.array([x * 4 * L for x in range(num_drones)]),
                      np.array([y * 4 * L for y in range(num_drones)]),
                      np.ones(num_drones) * (collision_h / 2 - collision_z_offset + .1)]).transpose().reshape(num_drones, 3)


def multihover_targets(init_xyzs):
    """MultiHoverAviary.py:71: TARGET_POS = INIT_XYZS + [0, 0, 1/(n+1)], [N, 3]"""
    init_xyzs = np.asarray(init_xyzs, float)
    return init_xyzs + np.array([[0, 0, 1 / (i + 1)] for i in range(init_xyzs.shape[0])])


def multihover_spaces(num_drones, act=ActionType.RPM, action_buffer_size=15):
    """(action_space, observation_space) of one env, shapes (N, A) and (N, 12 + B A)
    (BaseRLAviary.py:132-156, 243-277)"""
    size = _ACT_SIZE[act]
    lo, hi = -np.inf, np.inf
    low = [lo, lo, 0] + [lo] * 9 + [-1] * size * action_buffer_size
    high = [hi] * 12 + [+1] * size * action_buffer_size
    return (Box(low=-np.ones((num_drones, size)), high=np.ones((num_drones, size)), dtype=np.float32),
            Box(low=np.array([low] * num_drones), high=np.array([high] * num_drones), dtype=np.float32))


class MultiDroneHelpers:
    """What the envs with N drones per env share (MultiHoverAviary, CtrlAviary, VelocityAviary): the
    neighbourhood helpers and the introspection of the handle ``self.h``."""

    # ---- multi-drone helpers (torch, from the state snapshot: no kernel of their own) ----
    def close(self):
        self.h.close()

    def _positions(self):
        """[E, N, 3] drone positions (state snapshot columns e*N + n)"""
        if self._pos_rows is None:
            names = self.state_field_names()[0]
            self._pos_rows = [names.index(k) for k in ("pos_x", "pos_y", "pos_z")]
        f, _ = self.get_state()
        return f[self._pos_rows].reshape(3, self.num_envs, self.NUM_DRONES).permute(1, 2, 0)

    def adjacency_matrix(self):
        """BaseAviary._getAdjacencyMatrix per env: [E, N, N] of 0 / 1, adj[e, i, j] == 1 iff i == j or
        |pos_i - pos_j| < NEIGHBOURHOOD_RADIUS"""
        p = self._positions()
        dist = (p[:, :, None, :] - p[:, None, :, :]).norm(dim=-1)
        adj = (dist < self.NEIGHBOURHOOD_RADIUS).to(p.dtype)
        eye = torch.eye(self.NUM_DRONES, dtype=p.dtype, device=p.device)
        return torch.maximum(adj, eye.expand_as(adj))

    def min_pair_distance(self):
        """[E] the smallest centre distance between two drones of each env (inf for one drone).  Drone-drone
        contact is not modelled: below about 2 * 0.06 m (the collision cylinders' radii) the reference's
        Bullet would have resolved a contact that this env does not."""
        p = self._positions()
        N = self.NUM_DRONES
        if N < 2:
            return torch.full((self.num_envs,), float("inf"), dtype=p.dtype, device=p.device)
        dist = (p[:, :, None, :] - p[:, None, :, :]).norm(dim=-1)
        dist = dist + torch.diag(torch.full((N,), float("inf"), dtype=p.dtype, device=p.device))
        return dist.reshape(self.num_envs, -1).min(dim=1).values

    # ---- introspection (tests / teacher forcing) ----
    def get_state(self):
        """(float [nf, E*N], int32 [ni, E*N]): HoverAviary's fields, column e*N + n; the per-env ints
        are replicated on the env's columns"""
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
        """the step-kernel instantiation this env launches (include/adrp.h adrp_handle_kernel_name)"""
        return self.h.kernel_name()


class MultiHoverAviary(MultiDroneHelpers, AviaryEnv):
    """Batched counterpart of gym_pybullet_adrp.envs.MultiHoverAviary."""

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, num_drones: int = 2,
                 neighbourhood_radius: float = np.inf, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.PYB, pyb_freq: int = 240, ctrl_freq: int = 30, gui=False,
                 record=False, obs: ObservationType = ObservationType.KIN, act: ActionType = ActionType.RPM,
                 *, num_envs: int = 1, device: int = 0, precision: str = "fp64", seed: int = 0,
                 autoreset: bool = True, init_noise=None, env_offset: int = 0, link_frame_lag: bool = True):
        if drone_model != DroneModel.CF2X:
            raise ValueError("only DroneModel.CF2X (cf2x_IROS.urdf) is supported")
        if gui or record:
            raise ValueError("GUI / video recording are out of scope (DESIGN.md)")
        if obs != ObservationType.KIN:
            raise ValueError("only ObservationType.KIN is supported")
        if act not in _ACT_CODE:
            raise ValueError("MultiHoverAviary supports the action types RPM and ONE_D_RPM (PID, VEL and "
                             "ONE_D_PID are not supported)")
        if pyb_freq % ctrl_freq != 0:
            raise ValueError("[ERROR] in BaseAviary.__init__(), pyb_freq is not divisible by env_freq.")
        num_drones = int(num_drones)
        if not 1 <= num_drones <= abi.MAX_DRONES:
            raise ValueError(f"MultiHoverAviary num_drones must be 1..{abi.MAX_DRONES}")
        cfg = _lib.default_config(abi.TASK_MULTIHOVER)
        cfg.num_drones = num_drones
        cfg.physics = PHYSICS_CODE[physics]
        cfg.act_type = _ACT_CODE[act]
        cfg.num_envs = int(num_envs)
        cfg.pyb_freq, cfg.ctrl_freq = int(pyb_freq), int(ctrl_freq)
        cfg.action_buffer_size = int(ctrl_freq // 2)
        cfg.autoreset = 1 if autoreset else 0
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
        self.DRONE_MODEL, self.PHYSICS, self.OBS_TYPE, self.ACT_TYPE = drone_model, physics, obs, act
        self.NUM_DRONES = num_drones
        self.NEIGHBOURHOOD_RADIUS = neighbourhood_radius
        self.PYB_FREQ, self.CTRL_FREQ = int(pyb_freq), int(ctrl_freq)
        self.PYB_STEPS_PER_CTRL = self.PYB_FREQ // self.CTRL_FREQ
        self.PYB_TIMESTEP, self.CTRL_TIMESTEP = 1.0 / self.PYB_FREQ, 1.0 / self.CTRL_FREQ
        self.ACTION_BUFFER_SIZE = int(ctrl_freq // 2)
        self.INIT_XYZS, self.INIT_RPYS = init_xyzs, init_rpys
        self.TARGET_POS = multihover_targets(init_xyzs)
        self.EPISODE_LEN_SEC = 8
        self.M, self.L, self.KF, self.KM = d.m, d.l, d.kf, d.km
        self.J = np.diag([d.ixx, d.iyy, d.izz])
        self.G = cfg.gravity
        self.GRAVITY = self.G * self.M
        self.HOVER_RPM = np.sqrt(self.GRAVITY / (4 * self.KF))
        self.MAX_RPM = np.sqrt((d.thrust2weight * self.GRAVITY) / (4 * self.KF))
        self.num_envs = cfg.num_envs
        self.action_space = self._actionSpace()
        self.observation_space = self._observationSpace()
        E, N, D = self.num_envs, num_drones, self.h.D
        self._obs = torch.zeros((E, N, D), dtype=torch.float32, device=self.device)
        self._tobs = torch.zeros_like(self._obs)
        self._rew = torch.zeros(E, dtype=torch.float32, device=self.device)
        # the kernel writes 0/1 bytes: valid torch.bool storage, returned without a cast
        self._term = torch.zeros(E, dtype=torch.bool, device=self.device)
        self._trunc = torch.zeros(E, dtype=torch.bool, device=self.device)
        self._act_shape = (E, N, self.h.A)
        self._info = {"answer": 42, "terminal_observation": self._tobs}
        self.h.bind(self._obs, self._rew, self._term, self._trunc, self._tobs)
        self._pos_rows = None

    # ---- spaces (BaseRLAviary.py:132-156, 243-277) ----
    def _actionSpace(self):
        return multihover_spaces(self.NUM_DRONES, self.ACT_TYPE, self.ACTION_BUFFER_SIZE)[0]

    def _observationSpace(self):
        return multihover_spaces(self.NUM_DRONES, self.ACT_TYPE, self.ACTION_BUFFER_SIZE)[1]

    # ---- gymnasium-style API, batched ----
    def reset(self, seed: int = None, options: dict = None, mask=None):
        """Reset all envs (or those with mask[e] != 0, all N drones of each); `seed` re-keys the random
        streams first.  Returns (obs [E,N,D], info)."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if seed is not None:
            if m is not None:
                raise ValueError("reset(seed=...) re-keys every env: call it without a mask")
            self.h.reseed(seed)
        self.h.reset(self._obs, m)
        return self._obs, {"answer": 42}

    def step(self, action):
        """One env.step of every env: action [E,N,A] (torch or numpy, in [-1,1]).

        Returns views of persistent device buffers (obs [E,N,D], reward [E], terminated [E],
        truncated [E]) that the next step overwrites."""
        act = action
        if not (isinstance(act, torch.Tensor) and act.dtype == torch.float32 and act.device == self.device
                and act.is_contiguous() and act.shape == self._act_shape):
            act = torch.as_tensor(action, device=self.device, dtype=torch.float32).reshape(self._act_shape)
            act = act.contiguous()
        self.h.step_ptr(act.data_ptr())
        return self._obs, self._rew, self._term, self._trunc, self._info

    def bind_outputs(self, obs, rew, term, trunc, tobs=None):
        """Write step / reset outputs into caller-owned device tensors from now on: obs [E,N,D] float32,
        reward [E] float32, terminated / truncated [E] bool, optionally the terminal observations
        [E,N,D] float32, all contiguous on this env's device."""
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
