"""Batched GPU environments (HoverAviary, MultiHoverAviary, MultiRaceAviary)."""
from .hover import HoverAviary  # noqa: F401
from .multihover import MultiHoverAviary  # noqa: F401
from .race import MultiRaceAviary  # noqa: F401
