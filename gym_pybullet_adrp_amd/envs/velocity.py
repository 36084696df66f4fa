"""VelocityAviary on the GPU: E independent envs of N drones each, velocity commands in, drone state rows
out, stepped by one fused HIP launch.

Mirrors the reference surface (envs/VelocityAviary.py): the action of a drone is [direction 3, fraction of
SPEED_LIMIT 1]; one DSLPIDControl per drone, fused into the step kernel, is called once per env.step on
the state at the start of the step with target position = current position, target rpy = (0, 0, current
yaw) and target velocity SPEED_LIMIT |a3| a[0:3] / |a[0:3]| (float32 arithmetic on the float32 action, a
zero direction gives zero velocity); its RPMs drive all PYB_FREQ / CTRL_FREQ sub-steps and are the last
four columns of the observation row (envs/ctrl.py).  ``reset`` keeps the controllers' state (the pid_*
snapshot fields): the reference builds them once in the constructor and never resets them.

The reference's DSLPIDControl CF2X mixer was written for cf2x.urdf, whose prop 0 sits at (+x, -y);
DroneModel.CF2X here is cf2x_IROS.urdf with prop 0 at (+x, +y), so the roll loop is positive feedback and
the reference's own VelocityAviary tumbles within seconds.  This env reproduces it.
"""
import numpy as np

from ..utils import abi
from ..utils.spaces import Box
from .ctrl import StateRowAviary, _MAX_SPEED_KMH


def speed_limit(max_speed_kmh=_MAX_SPEED_KMH):
    """VelocityAviary.py:78"""
    return 0.03 * max_speed_kmh * (1000 / 3600)


def velocity_action_space(num_drones):
    """VelocityAviary.py:92-94, shape (N, 4)"""
    return Box(low=np.array([[-1, -1, -1, 0]] * num_drones), high=np.array([[1, 1, 1, 1]] * num_drones), dtype=np.float32)


class VelocityAviary(StateRowAviary):
    """Batched counterpart of gym_pybullet_adrp.envs.VelocityAviary."""

    TASK = abi.TASK_VELOCITY

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.SPEED_LIMIT = speed_limit(self.MAX_SPEED_KMH)

    def _actionSpace(self):
        return velocity_action_space(self.NUM_DRONES)
