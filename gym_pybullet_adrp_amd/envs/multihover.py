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

from ..utils import abi
from ..utils.enums import ActionType, DroneModel, ObservationType, Physics
from ..utils.spaces import Box
from .kin import KinAviary, default_init_xyzs   # noqa: F401 (default_init_xyzs: imported from here by others)

_ACT_CODE = {ActionType.RPM: abi.ACT_RPM, ActionType.ONE_D_RPM: abi.ACT_ONE_D_RPM}
_ACT_SIZE = {ActionType.RPM: 4, ActionType.ONE_D_RPM: 1}


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
    """What the envs with N drones per env share beside KinAviary (MultiHoverAviary, CtrlAviary,
    VelocityAviary): the neighbourhood helpers."""

    # ---- multi-drone helpers (torch, from the state snapshot: no kernel of their own) ----
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


class MultiHoverAviary(MultiDroneHelpers, KinAviary):
    """Batched counterpart of gym_pybullet_adrp.envs.MultiHoverAviary."""

    TASK = abi.TASK_MULTIHOVER

    def __init__(self, drone_model: DroneModel = DroneModel.CF2X, num_drones: int = 2,
                 neighbourhood_radius: float = np.inf, initial_xyzs=None, initial_rpys=None,
                 physics: Physics = Physics.PYB, pyb_freq: int = 240, ctrl_freq: int = 30, gui=False,
                 record=False, obs: ObservationType = ObservationType.KIN, act: ActionType = ActionType.RPM,
                 *, num_envs: int = 1, device: int = 0, precision: str = "fp64", seed: int = 0,
                 autoreset: bool = True, init_noise=None, env_offset: int = 0, link_frame_lag: bool = True):
        super().__init__(drone_model, num_drones, neighbourhood_radius, initial_xyzs, initial_rpys, physics, pyb_freq,
                         ctrl_freq, gui, record, obs, act, num_envs=num_envs, device=device, precision=precision,
                         seed=seed, autoreset=autoreset, init_noise=init_noise, env_offset=env_offset,
                         link_frame_lag=link_frame_lag)

    def _check_types(self, obs, act):
        if obs != ObservationType.KIN:
            raise ValueError("only ObservationType.KIN is supported")
        if act not in _ACT_CODE:
            raise ValueError("MultiHoverAviary supports the action types RPM and ONE_D_RPM (PID, VEL and "
                             "ONE_D_PID are not supported)")
        return _ACT_CODE[act]

    def _task_attributes(self, d):
        self.TARGET_POS = multihover_targets(self.INIT_XYZS)
        self.EPISODE_LEN_SEC = 8

    # ---- spaces (BaseRLAviary.py:132-156, 243-277) ----
    def _actionSpace(self):
        return multihover_spaces(self.NUM_DRONES, self.ACT_TYPE, self.ACTION_BUFFER_SIZE)[0]

    def _observationSpace(self):
        return multihover_spaces(self.NUM_DRONES, self.ACT_TYPE, self.ACTION_BUFFER_SIZE)[1]

    # ---- gymnasium-style API, batched (reset, bind_outputs: KinAviary) ----
    def step(self, action):
        """One env.step of every env: action [E,N,A] (torch or numpy, in [-1,1]).

        Returns views of persistent device buffers (obs [E,N,D], reward [E], terminated [E],
        truncated [E]) that the next step overwrites."""
        self.h.step_ptr(self._as_action(action, torch.float32).data_ptr())
        return self._obs, self._rew, self._term, self._trunc, self._info
