"""Batched GPU controllers (the reference's gym_pybullet_adrp.control, for CtrlAviary users)."""
from .DSLPIDControl import DSLPIDControl  # noqa: F401
from .MellingerControl import MellingerControl  # noqa: F401
