"""Batched GPU environments (HoverAviary, MultiHoverAviary, CtrlAviary, VelocityAviary, MultiRaceAviary)."""
from .ctrl import CtrlAviary  # noqa: F401
from .hover import HoverAviary  # noqa: F401
from .velocity import VelocityAviary  # noqa: F401
from .multihover import MultiHoverAviary  # noqa: F401
from .race import MultiRaceAviary  # noqa: F401
