"""Start formations and waypoint tables of the controller demos (tools/pid.py, the dslpid fixture).

The geometry is that of the reference's examples (examples/pid.py, examples/downwash.py), stated here as
arrays: positions [N, 3], attitudes [N, 3], a table of xy waypoints [W, 2] that every drone cycles through at
its own height, and the index [N] at which each drone starts in the table.
"""
import numpy as np

SLOTS = 6          # the circle has six evenly spaced start slots; drone k takes slot k
LAP_SEC = 10       # one lap of the circle
SWEEP_SEC = 5      # one period of the downwash sweep


def circle(num_drones, ctrl_freq, height, radius=0.3, climb=0.05):
    """Drones on a circle of `radius` that touches the origin from below (centre (0, -radius)), drone k a sixth of
    a turn after drone k - 1 and `climb` higher, yawed k quarter turns / N.  The table is one lap of that circle
    at ctrl_freq points per second, starting at drone 0; drone k enters it at its own slot."""
    k = np.arange(num_drones)
    centre = np.array([0.0, -radius])
    turn = (k / SLOTS) * 2 * np.pi + np.pi / 2
    xyzs = np.column_stack([radius * np.cos(turn) + centre[0], radius * np.sin(turn) + centre[1], height + k * climb])
    rpys = np.column_stack([np.zeros(num_drones), np.zeros(num_drones), k * (np.pi / 2) / num_drones])
    points = ctrl_freq * LAP_SEC
    lap = (np.arange(points) / points) * (2 * np.pi) + np.pi / 2
    table = np.column_stack([radius * np.cos(lap) + xyzs[0, 0], radius * np.sin(lap) - radius + xyzs[0, 1]])
    start = ((k * points / SLOTS) % points).astype(np.int64)
    return xyzs, rpys, table, start


def downwash(ctrl_freq, half_span=0.5):
    """Two level drones, the upper at (half_span, 0, 1) above the lower at (-half_span, 0, 0.5), both sweeping
    x = half_span cos along y = 0, half a period apart."""
    xyzs = np.array([[half_span, 0.0, 1.0], [-half_span, 0.0, 0.5]])
    points = ctrl_freq * SWEEP_SEC
    phase = 2 * np.pi * (np.arange(points) / points)
    table = np.column_stack([half_span * np.cos(phase), np.zeros(points)])
    return xyzs, np.zeros((2, 3)), table, np.array([0, points // 2], np.int64)


def advance(index, table):
    """the next index of every drone in a cyclic table"""
    return (index + 1) % table.shape[0]
