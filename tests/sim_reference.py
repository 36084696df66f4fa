"""Plain numpy / Python restatement of what csrc/sim_kernel.h keeps on the device for the batched race
evaluation (gym_pybullet_adrp_amd/sim.py; the reference loop is scripts/sim.py:68-108):

* ``RaceAccounts``: the per-run / per-drone results accounting of ``race_results_kernel``.  A wave opens envs
  ``e < n_open`` as runs ``base + e``; per step an open env adds its float32 reward to a float64 sum and counts
  the step, each drone's gates are copied and its first ``flags & 2`` (finished) / ``flags & 1`` (eliminated)
  step is kept; on ``term | trunc`` the run is logged and the env closes.  A closed env records nothing.
* ``policy_command_row``: the command row of an RLController drone (RLController._action_transform:
  ``[action[:3], ZERO3, ZERO3, action[3], ZERO3, self.time]``) in the commands.py layout.
* ``winner``: the drone with the smallest finish step, ties to the lower index, -1 if nobody finished.

The yardstick of tests/test_sim_gpu.py; pinned on a case computed by hand in tests/test_sim_abi.py.
"""
import numpy as np

CMD_FULLSTATE, CMD_ARGS, TIME_SLOT = 1, 14, 13


class RaceAccounts:
    def __init__(self, n_envs, n_drones, capacity):
        E, N, C = int(n_envs), int(n_drones), int(capacity)
        self.E, self.N, self.C = E, N, C
        self.open = np.zeros(E, bool)
        self.run_return = np.zeros(E)                       # float64
        self.run_length = np.zeros(E, np.int32)
        self.run_gates = np.zeros((E, N), np.int32)
        self.run_finish = np.full((E, N), -1, np.int32)
        self.run_elim = np.full((E, N), -1, np.int32)
        self.log_return = np.zeros(C)
        self.log_length = np.zeros(C, np.int32)
        self.log_term = np.zeros(C, np.uint8)
        self.log_trunc = np.zeros(C, np.uint8)
        self.log_gates = np.zeros((C, N), np.int32)
        self.log_finish = np.full((C, N), -1, np.int32)
        self.log_elim = np.full((C, N), -1, np.int32)
        self.logged = self.steps = 0
        self.base = 0

    def begin(self, base, n_open):
        assert 0 <= n_open <= self.E and base >= 0 and base + n_open <= self.C
        self.base = int(base)
        self.run_return[:] = 0
        self.run_length[:] = 0
        self.run_gates[:] = 0
        self.run_finish[:] = -1
        self.run_elim[:] = -1
        self.open[:] = np.arange(self.E) < n_open

    def step(self, gate, flags, rew, term, trunc):
        gate = np.asarray(gate, np.int32).reshape(self.E, self.N)
        flags = np.asarray(flags, np.int32).reshape(self.E, self.N)
        rew = np.asarray(rew, np.float32)
        for e in range(self.E):
            if not self.open[e]:
                continue
            self.run_return[e] += np.float64(rew[e])
            self.run_length[e] += 1
            for n in range(self.N):
                self.run_gates[e, n] = gate[e, n]
                if flags[e, n] & 2 and self.run_finish[e, n] < 0:
                    self.run_finish[e, n] = self.run_length[e]
                if flags[e, n] & 1 and self.run_elim[e, n] < 0:
                    self.run_elim[e, n] = self.run_length[e]
            if term[e] or trunc[e]:
                s = self.base + e
                self.log_return[s] = self.run_return[e]
                self.log_length[s] = self.run_length[e]
                self.log_term[s] = 1 if term[e] else 0
                self.log_trunc[s] = 1 if trunc[e] else 0
                self.log_gates[s] = self.run_gates[e]
                self.log_finish[s] = self.run_finish[e]
                self.log_elim[s] = self.run_elim[e]
                self.open[e] = False
                self.logged += 1
        self.steps += 1

    @property
    def remaining(self):
        return int(self.open.sum())

    def episode_times(self, ctrl_freq):
        return (self.log_length.astype(np.float64) - 1.0) / float(ctrl_freq)


def winner(finish_step):
    f = np.asarray(finish_step)
    out = np.full(f.shape[0], -1, np.int64)
    for r in range(f.shape[0]):
        best = None
        for n in range(f.shape[1]):
            if f[r, n] >= 0 and (best is None or f[r, n] < f[r, best]):
                best = n
        out[r] = -1 if best is None else best
    return out


def policy_command_row(setpoint, ep_time):
    """(code, float64 [14]) of one policy drone: setpoint = float32 (x, y, z, yaw)"""
    s = np.asarray(setpoint, np.float32)
    a = np.zeros(CMD_ARGS)
    a[0:3] = s[0:3].astype(np.float64)
    a[9] = np.float64(s[3])
    a[TIME_SLOT] = float(ep_time)
    return CMD_FULLSTATE, a


def results_stream(steps, n_envs, n_drones, seed, never=None):
    """constructed inputs of the results test: per step gate / flags [E, N] int32, rew [E] float32 (multiples of
    1/8: every partial sum is exact in float64), term / trunc [E] uint8.  Env 0 closes on step 1, env ``never``
    never closes, drone 0 of env 1 is eliminated and later also finished; the rest is random: flags are sticky
    bits, gates grow."""
    rng = np.random.default_rng(seed)
    E, N = n_envs, n_drones
    gate = np.zeros((steps, E, N), np.int32)
    flags = np.zeros((steps, E, N), np.int32)
    g, f = np.zeros((E, N), np.int32), np.zeros((E, N), np.int32)
    for t in range(steps):
        g = np.minimum(g + (rng.random((E, N)) < 0.15), 4).astype(np.int32)
        f = f | (rng.random((E, N)) < 0.04).astype(np.int32) | (2 * (g >= 4)).astype(np.int32)
        if E > 1 and t >= 2:
            f[1, 0] |= 1
        if E > 1 and t >= 5:
            f[1, 0] |= 2
        gate[t], flags[t] = g, f
    rew = (rng.integers(-40, 41, (steps, E)) / 8.0).astype(np.float32)
    term = (rng.random((steps, E)) < 0.03).astype(np.uint8)
    trunc = (rng.random((steps, E)) < 0.03).astype(np.uint8)
    term[0, 0] = 1
    if E > 1:                       # env 1 stays open until its drone 0 holds both bits
        term[:6, 1] = 0
        trunc[:6, 1] = 0
    if never is not None:
        term[:, never] = 0
        trunc[:, never] = 0
    return gate, flags, rew, term, trunc
