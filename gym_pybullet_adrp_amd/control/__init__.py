"""Batched GPU controllers (the reference's gym_pybullet_adrp.control, for CtrlAviary users)."""
from .DSLPIDControl import DSLPIDControl  # noqa: F401
